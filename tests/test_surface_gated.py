"""The face-normal gate of the surface search on the GPU (gate_on="surface"): face normals against float64, the gated search
against its fp32 transcription (bitwise), the culled sweep against the exhaustive one (bitwise), the open gate against the ungated
kernels, invariance under the split and under batching, the gradient against float64, a scan whose normals all point inward,
alignment / fit / registration under the gate, what stays untouched when the gate is off, and the argument errors."""
import functools
import os

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, editing, ops, scan
from semantichuman_amd.hierarchy import load_hierarchy
from tests import surface_gated_ref as G
from tests import surface_ref as R
from tests.launch_record import recorded
from tests.normals_ref import angle, bodies
from tests.test_scan import PARTS, semantic_setup

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
GATED_KERNELS = {"face_normals_kernel", "surface_prep_gated_kernel", "surface_search_gated_kernel", "surface_finish_gated_kernel"}
UV_TOL = 4 * 2.0 ** -24                                                    # the weights of test_surface.py's rule (c)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return all(torch.equal(bits(u), bits(v)) for u, v in zip(a, b))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def batch_of(case, order=None, scale=None, flip=True):
    """(x on the device, FaceTable, ScanBatch with normals, the host inputs) of G.case_inputs(*case)."""
    x, faces, n, counts, clouds, normals, vmask = G.case_inputs(*case, flip=flip)
    if scale is not None:
        clouds = [c * np.float32(scale) for c in clouds]
    return dev(x), scan.FaceTable(faces, n, DEV), scan.ScanBatch(clouds, DEV, order=order, normals=normals), (x, faces, n, counts, clouds, normals, vmask)


CASES = [(t, B, M, masked) for t in G.TEMPLATES for (B, M) in G.SHAPES for masked in (False, True)]
case_id = lambda c: "%s-B%d-M%d-m%d" % (c[0].split(".")[0], c[1], c[2], c[3])


# ------------------------------------------------------------------------------------------------ 1. face normals
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", G.TEMPLATES)
def test_face_normals_against_float64(name, B):
    x, f = bodies(name, B)
    n = x.shape[1] - 1
    x[:, n] = np.nan                                                       # the dummy row: a kernel that addressed it would show
    nrm = scan.face_normals(dev(x), f).cpu().numpy()
    assert nrm.shape == (B, f.shape[0], 3) and nrm.dtype == np.float32 and np.isfinite(nrm).all()
    worst = max(float(angle(nrm[b], G.face_normals_f64(x[b, :n], f)).max()) for b in range(B))
    bound = G.KERNEL_FACTOR * G.F32_FACE_ANGLE
    print("face_normals %s B=%d: largest angle to float64 %.3e rad = %.1f %% of the bound %.3e" % (name, B, worst, 100 * worst / bound, bound))
    assert worst <= bound
    for b in range(B):                                                     # and the transcription, bit for bit
        assert np.array_equal(nrm[b].view(np.int32), G.face_normals_f32(x[b, :n], f).view(np.int32)), b
    # a face with a corner outside [0, n) or without area: the zero normal, through the bare entry point
    table = dev(np.array([[0, 1, 2], [0, 1, n], [0, 1, -1], [3, 3, 4]], np.int32))
    got = ops.face_normals(dev(x), table, n).cpu().numpy()
    assert (np.abs(got[:, 0]).sum(-1) > 0).all() and (got[:, 1:] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. against the transcription
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gated_search_equals_the_transcription(case):
    """face and the bits of d2 are the fp32 transcription's (the exhaustive gated reference), uv within 4 x 2^-24, for the
    exhaustive and the culled sweep, at 30 / 60 / 90 / 180 degrees.  The conditions that keep the case from being vacuous are
    asserted on the reference itself."""
    xd, ft, sb, (x, faces, n, counts, clouds, normals, vmask) = batch_of(case)
    if case[2] >= 63:
        print("conditions %s: kept / none / differing = %s" % (case_id(case), G.check_conditions(*case)))
    for deg in G.ANGLES:
        ref = G.case_reference(*case, deg)
        for cull in (False, True):
            face, d2, uv = (t.cpu().numpy() for t in scan.nearest_surface(sb.points, xd, ft, q_count=sb.counts, vertex_mask=vmask, cull=cull,
                                                                            q_normals=sb.normals, normal_angle=deg))
            for b, m in enumerate(counts):
                rf, rd, ruv = ref[b]
                assert np.array_equal(face[b, :m], rf), (deg, cull, b, int((face[b, :m] != rf).sum()))
                assert np.array_equal(d2[b, :m].view(np.int32), rd.view(np.int32)), (deg, cull, b)
                assert float(np.abs(uv[b, :m] - ruv).max()) <= UV_TOL, (deg, cull, b)
                assert (uv[b, :m][rf < 0] == 0).all() and np.isinf(d2[b, :m][rf < 0]).all()
                assert (face[b, m:] == -1).all() and (d2[b, m:] == 0).all() and (uv[b, m:] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. the cull is exact
@pytest.mark.parametrize("case", CASES + [("template6890.npz", 16, 20011, False)], ids=case_id)
def test_gated_cull_equals_the_full_sweep_bitwise(case):
    for scale in (None, 3.0):
        for order in (None, "morton"):
            xd, ft, sb, (x, faces, n, counts, clouds, normals, vmask) = batch_of(case, order, scale)
            for deg in (60.0,) if case[2] > 1000 else (30.0, 60.0, 90.0):
                full = scan.nearest_surface(sb.points, xd, ft, q_count=sb.counts, vertex_mask=vmask, cull=False, q_normals=sb.normals,
                                            normal_angle=deg)
                culled = scan.nearest_surface(sb.points, xd, ft, q_count=sb.counts, vertex_mask=vmask, cull=True, q_normals=sb.normals,
                                              normal_angle=deg)
                assert same(full, culled), (scale, order, deg)


# ------------------------------------------------------------------------------------------------ 4. the open gate
def test_angle_180_gives_the_ungated_bits_through_the_new_kernels():
    case = ("template6890.npz", 3, 1000, True)
    xd, ft, sb, (x, faces, n, counts, clouds, normals, vmask) = batch_of(case)
    base = scan.nearest_surface(sb.points, xd, ft, q_count=sb.counts, vertex_mask=vmask)
    for cull in (True, False):
        got, names = recorded(lambda: scan.nearest_surface(sb.points, xd, ft, q_count=sb.counts, vertex_mask=vmask, cull=cull,
                                                           q_normals=sb.normals, normal_angle=180))
        assert same(base, got), cull
        assert GATED_KERNELS <= names and "surface_search_kernel" not in names and "surface_finish_kernel" not in names, sorted(names)
    trunc = 0.05
    for w in (0.0, 0.5):
        xa, xb = xd.clone().requires_grad_(True), xd.clone().requires_grad_(True)
        La = scan.chamfer(xa, sb, vertex_mask=vmask, trunc=trunc, w_model_to_scan=w, faces=ft)
        Lb = scan.chamfer(xb, sb, vertex_mask=vmask, trunc=trunc, w_model_to_scan=w, faces=ft, normal_angle=180, gate_on="surface")
        ga, = torch.autograd.grad(La.sum(), xa)
        gb, = torch.autograd.grad(Lb.sum(), xb)
        assert torch.equal(bits(La.detach()), bits(Lb.detach())) and torch.equal(bits(ga), bits(gb)), w
        L60 = scan.chamfer(xd, sb, vertex_mask=vmask, trunc=trunc, w_model_to_scan=w, faces=ft, normal_angle=60, gate_on="surface")
        assert not torch.equal(L60, La.detach())                           # at 60 degrees the flipped normals do change the loss


# ------------------------------------------------------------------------------------------------ 5. invariance
def test_gated_splitting_and_batching_are_invisible():
    x, faces, n, counts, clouds, normals, vmask = G.case_inputs("template6890.npz", 16, 20011, False)
    cloud, nrm = clouds[0], normals[0]
    xd = dev(x)
    ft = scan.FaceTable(faces, n, DEV)
    one = scan.ScanBatch([cloud], DEV, order="morton", normals=[nrm])
    rs = np.random.RandomState(4)
    others = [rs.randn(int(m), 3).astype(np.float32) for m in rs.randint(1, 20011, size=15)]
    onrm = [rs.randn(o.shape[0], 3) for o in others]
    many = scan.ScanBatch(others[:5] + [cloud] + others[5:], DEV, order="morton", normals=onrm[:5] + [nrm] + onrm[5:])
    x16 = xd.clone()
    x16[5] = xd[0]
    assert _lib.load().sh_nearest_surface_chunks(1, 20011, faces.shape[0]) > 1
    cos_min = G.cos_min_of(60.0)
    fn1 = ops.face_normals(xd[:1], ft.faces, n)
    ref = ops.nearest_surface(one.points, xd[:1], ft.faces, n, one.counts, chunks=1, gate=(one.normals, fn1, cos_min))
    assert int((ref[0][0] < 0).sum()) > 0 and int((ref[0][0] >= 0).sum()) > 10000
    for chunks in (0, 2, 7, 79):
        for cull in (True, False) if chunks in (0, 7) else (True,):
            got = ops.nearest_surface(one.points, xd[:1], ft.faces, n, one.counts, chunks=chunks, cull=cull, gate=(one.normals, fn1, cos_min))
            assert same(ref, got), (chunks, cull)
    batched = scan.nearest_surface(many.points, x16, ft, q_count=many.counts, q_normals=many.normals, normal_angle=60)
    m = cloud.shape[0]
    assert same([t[0, :m] for t in ref], [t[5, :m] for t in batched])
    for w in (0.0, 0.5):                                                   # loss and gradient: alone against one of 16
        xa = xd[:1].clone().requires_grad_(True)
        xb = x16.clone().requires_grad_(True)
        La = scan.chamfer(xa, one, trunc=0.02, w_model_to_scan=w, faces=ft, normal_angle=60, gate_on="surface")
        Lb = scan.chamfer(xb, many, trunc=0.02, w_model_to_scan=w, faces=ft, normal_angle=60, gate_on="surface")
        ga, = torch.autograd.grad(La.sum(), xa)
        gb, = torch.autograd.grad(Lb.sum(), xb)
        assert torch.equal(bits(La[0]), bits(Lb[5])) and torch.equal(bits(ga[0]), bits(gb[5])), w
        assert float(ga.abs().max()) > 0 and float(ga[0, n:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 6. gradient
@pytest.mark.parametrize("w", [0.0, 0.5])
def test_gated_surface_chamfer_gradient_against_float64(w):
    """scan.chamfer(..., gate_on="surface") backward against surface_ref.surface_grad_f64 evaluated on the recorded (face, uv) with
    the kept set of the gated result (a face, and d2 < trunc^2): max|g - g64| <= 4 x F32_GRAD_REL x max|g64| per body."""
    case = ("template6890.npz", 3, 1000, True)
    xd, ft, sb, (x, faces, n, counts, clouds, normals, vmask) = batch_of(case)
    B, trunc = 3, 0.02
    tau2 = np.float32(trunc ** 2)
    n_act = int(vmask.sum())
    xg = xd.clone().requires_grad_(True)
    matches = {}
    L = scan.chamfer(xg, sb, vertex_mask=vmask, trunc=trunc, w_model_to_scan=w, faces=ft, normal_angle=60, gate_on="surface", matches=matches)
    gL = dev(np.random.RandomState(2).randn(B).astype(np.float32))
    g, = torch.autograd.grad(L, xg, gL)
    gn, gLn = g.cpu().numpy(), gL.cpu().numpy().astype(np.float64)
    face, uv, d2 = (matches[k].cpu().numpy() for k in ("face", "uv", "d2_surface"))
    assert set(matches) >= {"x", "n", "v_mask", "mask_sb", "tau2", "w_ms", "idx_sm", "d2_sm", "idx_ms", "d2_ms", "face", "uv", "d2_surface",
                            "faces", "tn", "normal_faces"}
    ref = G.case_reference(*case, 60.0)
    # the recorded vertex matches are the gated vertex search's
    tn = scan.vertex_normals(xd, ft)
    i_sm, d_sm = ops.nearest_points(sb.points, xd, q_count=sb.counts, t_mask=vmask, nt=n, gate=(sb.normals, tn, G.cos_min_of(60.0)))
    assert same((matches["idx_sm"], matches["d2_sm"]), (i_sm, d_sm)) and same((matches["tn"],), (tn,))
    if w > 0:
        i_ms, d_ms = (t.cpu().numpy() for t in (matches["idx_ms"], matches["d2_ms"]))
    for b, m in enumerate(counts):
        assert np.array_equal(face[b, :m], ref[b][0])
        keep = (face[b, :m] >= 0) & (d2[b, :m] < tau2)
        assert 0 < keep.sum() < m
        g64 = np.zeros((x.shape[1], 3))
        g64[:n] = R.surface_grad_f64(clouds[b], x[b, :n], faces, np.where(keep, face[b, :m], 0), uv[b, :m], keep, n, m)
        if w > 0:
            on = np.zeros(x.shape[1], bool)
            on[:n] = vmask & (i_ms[b, :n] >= 0) & (d_ms[b, :n] < tau2)
            kk = np.nonzero(on)[0]
            g64[kk] += w * (2.0 / n_act) * (x[b, kk].astype(np.float64) - clouds[b][i_ms[b, kk]].astype(np.float64))
        g64 *= gLn[b]
        err, top = np.abs(gn[b] - g64).max(), np.abs(g64).max()
        print("gated surface gradient b=%d w=%g: max err %.3g of max|g| %.3g (%.3g; bound %.3g)"
              % (b, w, err, top, err / top, R.KERNEL_FACTOR * R.F32_GRAD_REL))
        assert err <= R.KERNEL_FACTOR * R.F32_GRAD_REL * top, (b, err, top)
        assert float(np.abs(gn[b, n:]).max()) == 0.0 and float(np.abs(gn[b, :n][~vmask]).max()) == 0.0


# ------------------------------------------------------------------------------------------------ 7. an inward scan
def test_an_all_inward_scan_is_truncated_and_never_swept_again():
    """The template itself (smooth and star-shaped, unlike the crumpled synth_batch bodies, on which a negated normal still
    finds a compatible face next door) and a copy 1.1 times its size, noise-free samples of each one's OWN surface, every normal
    negated, 60 degrees.  The compatible faces lie across the body (0.086 away at the least, measured on the host reference):
    with trunc = 0.05 every point is truncated, the loss is trunc^2, the gradient zero.  The finishing kernel must not sweep a
    point again only because it has no face: the counter of swept-again points is 0, also for a scan that has no compatible face
    at all (zero normals: bound +inf for every point)."""
    h = load_hierarchy(os.path.join(GOLD, "template6890.npz"))
    faces = np.asarray(h.faces, np.int64)
    v = np.asarray(h.verts, np.float32)
    n = v.shape[0]
    x = np.zeros((2, n + 1, 3), np.float32)
    x[0, :n], x[1, :n] = v, v * np.float32(1.1)
    clouds, normals = [], []
    for b in range(2):
        p, f = G.sample_surface_faces(x[b, :n], faces, 5000 - 7 * b, seed=40 + b)
        clouds.append(p)
        normals.append(-G.face_normals_f64(x[b, :n], faces)[f])
    sb = scan.ScanBatch(clouds, DEV, order="morton", normals=normals)
    xd, ft = dev(x), scan.FaceTable(faces, n, DEV)
    trunc = 0.05
    xg = xd.clone().requires_grad_(True)
    L = scan.chamfer(xg, sb, trunc=trunc, faces=ft, normal_angle=60, gate_on="surface")
    g, = torch.autograd.grad(L.sum(), xg)
    face, d2, uv = scan.nearest_surface(sb.points, xd, ft, q_count=sb.counts, q_normals=sb.normals, normal_angle=60)
    live = torch.arange(sb.points.shape[1], device=DEV)[None, :] < sb.counts[:, None]
    assert bool((d2[live] >= trunc ** 2).all())
    assert np.array_equal(L.detach().cpu().numpy(), np.full(2, np.float32(trunc ** 2)))      # every term is tau2, and so is their mean
    assert float(g.abs().max()) == 0.0
    # a gate nothing passes (every scan normal zero, 60 degrees): no face at all, bound +inf for every point - none swept again
    zero = scan.ScanBatch(clouds, DEV, order="morton", normals=[np.zeros_like(c, dtype=np.float64) for c in clouds])
    for nrm, none_at_all in ((sb.normals, False), (zero.normals, True)):
        stats = torch.zeros(2, dtype=torch.int64, device=DEV)
        fn = ops.face_normals(xd, ft.faces, n)
        f2, dd, _ = ops.nearest_surface(sb.points, xd, ft.faces, n, sb.counts, gate=(nrm, fn, G.cos_min_of(60.0)), stats=stats)
        tested, again = (int(v) for v in stats.cpu())
        print("inward scan (no face at all: %s): %d region tests, %d points swept again" % (none_at_all, tested, again))
        assert again == 0
        if none_at_all:
            assert bool((f2[live] == -1).all()) and bool(torch.isinf(dd[live]).all()) and tested == 0
        else:
            assert same((f2, dd), (face, d2))


# ------------------------------------------------------------------------------------------------ 8. align / fit / register
@functools.lru_cache(maxsize=None)
def fit_setup():
    m, z0, z_kps, dummy, _, x_star, n = semantic_setup()
    faces = np.asarray(load_hierarchy(os.path.join(GOLD, "semantic.npz")).faces, np.int64)
    xs = x_star.cpu().numpy()
    clouds, normals = [], []
    for b in range(3):
        p, f = G.sample_surface_faces(xs[b, :n], faces, 3000 - 11 * b, seed=60 + b, sigma=0.002)
        nr = G.face_normals_f64(xs[b, :n], faces)[f]
        nr[np.arange(len(f)) % 7 == 3] *= -1.0
        clouds.append(p)
        normals.append(nr)
    trunc = 0.25 * float(x_star[:, :n].abs().max())
    return m, z0, z_kps, dummy, x_star, n, faces, clouds, normals, trunc


def test_align_fit_and_register_under_the_gate():
    m, z0, z_kps, dummy, x_star, n, faces, clouds, normals, trunc = fit_setup()
    sb = scan.ScanBatch(clouds, DEV, order="morton", normals=normals)
    ft = scan.FaceTable(faces, n, DEV)
    gate = dict(faces=ft, normal_angle=60, gate_on="surface", trunc=trunc)

    def run():
        out = []
        for step in ("point", "plane"):
            for w in (0.0, 1.0):
                pose, aligned, log = scan.align(x_star, sb, mode="rigid", iters=3, init="identity", w_model_to_scan=w, step=step, **gate)
                out += [pose.packed, pose.scale, aligned.points, aligned.normals, log]
        # pose_update on gated matches, surface and vertex pairs
        for surface in (True, False):
            for step in ("point", "plane"):
                matches = {}
                scan.chamfer(x_star, sb, w_model_to_scan=0.5, matches=matches, **gate)
                pose = scan.Pose.identity(3, DEV)
                aligned = pose.apply(sb)
                scan.pose_update(pose, sb, aligned, matches, "rigid", surface=surface, step=step)
                out += [pose.packed, aligned.points]
        zf, final, losses = editing.fit_scan(m, z0, z_kps, sb, parts=PARTS, steps=1, lr=1e-2, w_model_to_scan=0.5, dummy=dummy, **gate)
        out += [zf, final, losses]
        for align_on in ("vertices", "surface"):
            for align_step in ("point", "plane"):
                zr, pose, final, losses = editing.register_scan(m, z0, z_kps, sb, parts=PARTS, mode="rigid", init="identity", align_iters=2,
                                                                steps=1, lr=1e-2, w_model_to_scan=0.5, dummy=dummy, align_on=align_on,
                                                                align_step=align_step, **gate)
                out += [zr, pose.packed, final, losses]
        return out

    a, names = recorded(run)
    b = run()
    assert GATED_KERNELS <= names and "surface_search_kernel" not in names, sorted(names)
    assert all(bool(torch.isfinite(t).all()) for t in a)
    assert same(a, b)


# ------------------------------------------------------------------------------------------------ 9. off means off
def entry_points(sb, ft, x_star, m, z0, z_kps, dummy, trunc, **kw):
    x = (x_star.detach() * 1.02).requires_grad_(True)
    loss = scan.chamfer(x, sb, trunc=trunc, w_model_to_scan=0.5, faces=ft, **kw)
    loss.sum().backward()
    ns = scan.nearest_surface(sb.points, x_star, ft, q_count=sb.counts)
    pose, aligned, log = scan.align(x_star, sb, mode="similarity", iters=3, trunc=trunc, faces=ft, **kw)
    fit = editing.fit_scan(m, z0, z_kps, sb, parts=PARTS, steps=1, lr=1e-2, w_model_to_scan=0.5, trunc=trunc, dummy=dummy, faces=ft, **kw)
    vert = scan.chamfer(x_star, sb, trunc=trunc, w_model_to_scan=0.5, **kw)
    return [loss.detach(), x.grad, *ns, pose.packed, pose.scale, aligned.points, log, *fit, vert]


def test_off_means_off():
    """Without gate_on="surface" every entry point launches what it launched and returns the same bits: calls that do not pass
    the argument, on scans without normals, against calls with gate_on="vertices" spelled out on scans that carry normals."""
    m, z0, z_kps, dummy, x_star, n, faces, clouds, normals, trunc = fit_setup()
    ft = scan.FaceTable(faces, n, DEV)
    bare = scan.ScanBatch(clouds, DEV, order="morton")
    with_n = scan.ScanBatch(clouds, DEV, order="morton", normals=normals)
    base, base_names = recorded(lambda: entry_points(bare, ft, x_star, m, z0, z_kps, dummy, trunc))
    got, names = recorded(lambda: entry_points(with_n, ft, x_star, m, z0, z_kps, dummy, trunc, gate_on="vertices"))
    assert same(base, got)
    assert names == base_names and not (names & GATED_KERNELS) and "nearest_search_gated_kernel" not in names, sorted(names)
    assert {"surface_prep_kernel", "surface_search_kernel", "surface_finish_kernel", "surface_bwd_kernel", "nearest_search_kernel"} <= names


# ------------------------------------------------------------------------------------------------ 10. errors
def test_gate_on_errors():
    xd, ft, sb, (x, faces, n, counts, clouds, normals, vmask) = batch_of(("small_ae.npz", 3, 63, False))
    bare = scan.ScanBatch(clouds, DEV)
    ok = dict(faces=ft, normal_angle=60, trunc=0.1, gate_on="surface")
    for fn in (lambda **k: scan.chamfer(xd, k.pop("scans", sb), **k), lambda **k: scan.align(xd, k.pop("scans", sb), iters=1, **k)):
        fn(**ok)
        with pytest.raises(ValueError, match="gate_on must be"):
            fn(**dict(ok, gate_on="faces"))
        with pytest.raises(ValueError, match="gate_on must be"):
            fn(gate_on="normals")
        with pytest.raises(ValueError, match="normal_angle"):
            fn(**dict(ok, normal_angle=None))
        with pytest.raises(ValueError, match="faces="):
            fn(**dict(ok, faces=None))
        with pytest.raises(ValueError, match="scan normals"):
            fn(**dict(ok, scans=bare))
        with pytest.raises(ValueError, match="trunc"):
            fn(**dict(ok, trunc=None))
        with pytest.raises(ValueError, match="normal_angle must lie"):
            fn(**dict(ok, normal_angle=0))
        with pytest.raises(ValueError, match="made for"):
            fn(**dict(ok, normal_faces=scan.FaceTable(faces[faces.max(1) < n - 1], n - 1, DEV)))
        fn(**dict(ok, normal_faces=faces))                                  # given, and describing the same n
        with pytest.raises(ValueError, match="not built"):                  # the gate on vertex normals stays what it was
            fn(**dict(ok, gate_on="vertices", normal_faces=ft))
    with pytest.raises(ValueError, match="come together"):
        scan.nearest_surface(sb.points, xd, ft, q_normals=sb.normals)
    with pytest.raises(ValueError, match="normal_angle must lie"):
        scan.nearest_surface(sb.points, xd, ft, q_normals=sb.normals, normal_angle=181)
    fn32 = ops.face_normals(xd, ft.faces, n)
    with pytest.raises(RuntimeError, match="cos_min is NaN"):
        ops.nearest_surface(sb.points, xd, ft.faces, n, sb.counts, gate=(sb.normals, fn32, float("nan")))
    with pytest.raises(RuntimeError, match="face normals"):
        ops.nearest_surface(sb.points, xd, ft.faces, n, sb.counts, gate=(sb.normals, fn32[:, :-1], 0.5))
