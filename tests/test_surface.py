"""Point-to-surface fitting on the GPU: the culled search against the unculled one (bitwise), against float64, its invariance
under the split of the triangle range and under batching, edge cases, the gradient against float64, the unchanged vertex path,
what the surface objective buys on surface-sampled scans, and one fit at the size tools/bench_surface.py times."""
import functools
import os

import numpy as np
import pytest
import torch

import semantichuman_amd as sh
from semantichuman_amd import _lib, editing, ops, scan, synthetic
from semantichuman_amd.hierarchy import load_hierarchy
from tests import scan_ref
from tests import surface_ref as R
from tests.test_scan import PARTS, semantic_setup, snapshot

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
SURFACE_KERNELS = {"surface_prep_kernel", "surface_search_kernel", "surface_finish_kernel", "surface_bwd_kernel"}


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return all(torch.equal(bits(u), bits(v)) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. the cull is exact
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("M", [1, 63, 1000, 20011])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("template", ["template6890.npz", "small_ae.npz"])
def test_cull_equals_the_full_sweep_bitwise(template, B, M, masked):
    for kind in ("s0", "s01", "far"):
        x, faces, n, counts, clouds, vmask = R.case_inputs(template, B, M, masked, kind)
        xd = torch.from_numpy(x).to(DEV)
        ft = scan.FaceTable(faces, n, DEV)
        for order in (None, "morton"):
            sb = scan.ScanBatch(clouds, DEV, order=order)
            full = scan.nearest_surface(sb.points, xd, ft, q_count=sb.counts, vertex_mask=vmask, cull=False)
            culled = scan.nearest_surface(sb.points, xd, ft, q_count=sb.counts, vertex_mask=vmask, cull=True)
            assert same(full, culled), (kind, order)
            face = culled[0].cpu().numpy()
            for b, m in enumerate(counts):
                assert (face[b, :m] >= 0).all() and (face[b, m:] == -1).all()


# ------------------------------------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("case", R.FLOAT64_CASES, ids=lambda c: "%s-B%d-M%d-m%d-%s" % (c[0].split(".")[0], c[1], c[2], c[3], c[4]))
def test_against_float64(case):
    """(a) |d2 - d2_64| <= 2 sqrt(d2_64) delta + delta^2; (b) the point rebuilt in float64 from the GPU's own (face, uv) lies at a
    squared distance from s that meets the same bound against the GPU's d2; (c) weights in [0, 1], summing to 1 within 4 ulp.
    delta = KERNEL_FACTOR * F32_DELTA_MULTIPLE * 2^-24 * max|coordinate| (tests/surface_ref.py says where the multiple comes
    from).  Faces are not compared; no query is exempt."""
    template, B, M, masked, kind = case
    x, faces, n, counts, clouds, vmask = R.case_inputs(template, B, M, masked, kind)
    xd = torch.from_numpy(x).to(DEV)
    sb = scan.ScanBatch(clouds, DEV)
    face, d2, uv = (t.cpu().numpy() for t in scan.nearest_surface(sb.points, xd, scan.FaceTable(faces, n, DEV), q_count=sb.counts,
                                                                    vertex_mask=vmask))
    worst = 0.0
    for b, m in enumerate(counts):
        s, xb = clouds[b], x[b, :n]
        f64, d64, _ = R.closest_f64(s, xb, faces, vmask)
        delta = R.KERNEL_FACTOR * R.F32_DELTA_MULTIPLE * 2.0 ** -24 * max(np.abs(xb).max(), np.abs(s).max())
        dg = d2[b, :m].astype(np.float64)
        fb, uvb = face[b, :m], uv[b, :m]
        assert (fb >= 0).all() and (fb < faces.shape[0]).all()
        if vmask is not None:
            assert vmask[faces[fb]].all()
        err_a = np.abs(dg - d64)
        assert (err_a <= R.delta_bound(d64, delta)).all(), ("(a)", b, float((err_a / R.delta_bound(d64, delta)).max()))
        d_re = ((s.astype(np.float64) - R.rebuild_f64(xb, faces, fb, uvb)) ** 2).sum(1)
        err_b = np.abs(d_re - dg)
        assert (err_b <= R.delta_bound(dg, delta)).all(), ("(b)", b, float((err_b / R.delta_bound(dg, delta)).max()))
        l0 = (np.float32(1) - uvb[:, 0]) - uvb[:, 1]
        assert (uvb >= 0).all() and (uvb <= 1).all() and (l0 >= 0).all() and (l0 <= 1).all()
        total = l0.astype(np.float64) + uvb[:, 0].astype(np.float64) + uvb[:, 1].astype(np.float64)
        assert (np.abs(total - 1.0) <= 4 * 2.0 ** -24).all(), "(c)"
        worst = max(worst, float((err_a / R.delta_bound(d64, delta)).max()), float((err_b / R.delta_bound(dg, delta)).max()))
    print("against float64 %s: worst share of the bound used %.3f" % (case, worst))


# ------------------------------------------------------------------------------------------------ 3. invariance
def test_triangle_range_splitting_and_batching_are_invisible():
    x, faces, n, counts, clouds, vmask = R.case_inputs("template6890.npz", 16, 20011, False, "s01")
    cloud = clouds[0]
    xd = torch.from_numpy(x).to(DEV)
    ft = scan.FaceTable(faces, n, DEV)
    one = scan.ScanBatch([cloud], DEV, order="morton")
    rs = np.random.RandomState(4)
    others = [rs.randn(int(m), 3).astype(np.float32) for m in rs.randint(1, 20011, size=15)]
    many = scan.ScanBatch(others[:5] + [cloud] + others[5:], DEV, order="morton")          # body 5 of 16, padded batch, ragged
    x16 = xd.clone()
    x16[5] = xd[0]
    assert _lib.load().sh_nearest_surface_chunks(1, 20011, faces.shape[0]) > 1
    bound = ops.nearest_points(one.points, xd[:1], q_count=one.counts, nt=n)[1]
    ref = ops.nearest_surface(one.points, xd[:1], ft.faces, n, one.counts, None, bound, chunks=1)
    for chunks in (0, 2, 7, 79):
        for cull in (True, False) if chunks in (0, 7) else (True,):
            got = ops.nearest_surface(one.points, xd[:1], ft.faces, n, one.counts, None, bound if cull else None, chunks=chunks, cull=cull)
            assert same(ref, got), (chunks, cull)
    batched = scan.nearest_surface(many.points, x16, ft, q_count=many.counts)
    m = cloud.shape[0]
    assert same([t[0, :m] for t in ref], [t[5, :m] for t in batched])
    # loss and gradient: the body alone against the same body as one of 16
    for w, trunc in ((0.0, None), (0.5, 0.02)):
        xa = xd[:1].clone().requires_grad_(True)
        xb = x16.clone().requires_grad_(True)
        La = scan.chamfer(xa, one, trunc=trunc, w_model_to_scan=w, faces=ft)
        Lb = scan.chamfer(xb, many, trunc=trunc, w_model_to_scan=w, faces=ft)
        ga, = torch.autograd.grad(La.sum(), xa)
        gb, = torch.autograd.grad(Lb.sum(), xb)
        assert torch.equal(bits(La[0]), bits(Lb[5])) and torch.equal(bits(ga[0]), bits(gb[5])), (w, trunc)
        assert float(ga.abs().max()) > 0 and float(ga[0, n:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 4. edge cases
def test_degenerate_faces_masks_empty_bodies_and_the_dummy_row():
    h = load_hierarchy(os.path.join(GOLD, "small_ae.npz"))
    v, faces = np.asarray(h.verts, np.float64), np.asarray(h.faces, np.int64)
    n = v.shape[0]
    x = scan_ref.model_points(v, 4, seed=1)
    # body 1: faces 0 and 1 collapse (a point, and two equal corners); the scan has points right at them
    f0, f1 = faces[0], faces[1]
    x[1, f0[1]] = x[1, f0[0]]; x[1, f0[2]] = x[1, f0[0]]
    x[1, f1[1]] = x[1, f1[0]]
    xd = torch.from_numpy(x).to(DEV)
    ft = scan.FaceTable(faces, n, DEV)
    clouds = [R.sample_surface(x[b, :n], faces, 300, seed=b, sigma=0.01) for b in range(4)]
    clouds[1][:3] = x[1, [f0[0], f1[0], f1[2]]]
    sb = scan.ScanBatch(clouds, DEV)
    only = torch.from_numpy(faces[:2].astype(np.int32)).to(DEV)             # a table of the two degenerate faces alone
    for cull in (True, False):
        face, d2, uv = ops.nearest_surface(sb.points[1:2], xd[1:2], only, n, cull=cull)
        assert (face >= 0).all() and torch.isfinite(d2).all() and (uv >= 0).all() and (uv.sum(-1) <= 1).all()
    face, d2, uv = scan.nearest_surface(sb.points, xd, ft)
    assert (face >= 0).all() and torch.isfinite(d2).all() and (uv >= 0).all() and (uv.sum(-1) <= 1).all()
    assert same(scan.nearest_surface(sb.points, xd, ft, cull=False), (face, d2, uv))
    assert float(d2[1, :3].max()) == 0.0
    # all faces of body 2 masked -> -1 / +inf / 0; m_b = 0 for body 3; counts cut body 0
    mask = torch.ones((4, n), dtype=torch.bool, device=DEV)
    mask[2] = False
    for cull in (True, False):
        face, d2, uv = scan.nearest_surface(sb.points, xd, ft, q_count=[5, 300, 300, 0], vertex_mask=mask, cull=cull)
        assert (face[0, :5] >= 0).all() and (face[0, 5:] == -1).all() and (d2[0, 5:] == 0).all()
        assert (face[2] == -1).all() and torch.isinf(d2[2]).all() and (d2[2] > 0).all() and (uv[2] == 0).all()
        assert (face[3] == -1).all() and (d2[3] == 0).all() and (uv[3] == 0).all()
    # a chamfer over that batch: finite where it should be, zero for the empty body, gradient finite
    xg = xd.clone().requires_grad_(True)
    cut = scan.ScanBatch.__new__(scan.ScanBatch)
    cut.points, cut.perm = sb.points, None
    cut.host_counts = np.array([5, 300, 300, 0], np.int32)
    cut.counts = torch.tensor([5, 300, 300, 0], dtype=torch.int32, device=DEV)
    L = scan.chamfer(xg, cut, faces=ft)
    g, = torch.autograd.grad(L.sum(), xg)
    assert torch.isfinite(L).all() and float(L[3].detach()) == 0.0 and torch.isfinite(g).all() and float(g[3].abs().max()) == 0.0
    # a face table that touches the dummy row is refused; M = 1 works
    with pytest.raises(ValueError):
        scan.chamfer(xd, sb, faces=np.array([[0, 1, n]]))
    with pytest.raises(ValueError):
        scan.FaceTable(np.array([[0, 1, n]]), n, DEV)
    face, d2, uv = scan.nearest_surface(sb.points[:, :1].contiguous(), xd, ft)
    assert tuple(face.shape) == (4, 1) and (face >= 0).all()
    # closest_points rebuilds the foot points: their distance to the scan is the search's d2
    face, d2, uv = scan.nearest_surface(sb.points, xd, ft)
    p = scan.closest_points(xd, ft, face, uv)
    assert float(((sb.points - p).pow(2).sum(-1) - d2).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------------ 5. gradient
@functools.lru_cache(maxsize=None)
def _grad_reference():
    x, faces, n, counts, clouds, vmask = R.grad_inputs()
    out = []
    for b, m in enumerate(counts):
        s, xb = clouds[b], x[b, :n]
        f64, d64, uv64 = R.closest_f64(s, xb, faces, vmask)
        tie = R.tie_mask_f64(s, xb, faces, f64, uv64, d64, vmask)
        out.append((f64, d64, uv64, tie))
    return x, faces, n, counts, clouds, vmask, out


@pytest.mark.parametrize("truncate", [False, True])
@pytest.mark.parametrize("w", [0.0, 0.5])
def test_surface_chamfer_gradient_against_float64(w, truncate):
    """scan.chamfer(..., faces=) backward against the float64 formula on the float64 search's own foot points:
    max|g - g64| <= KERNEL_FACTOR * F32_GRAD_REL * max|g64| per body.  Points within TIE of a medial-axis tie are left out on
    both sides (their share printed and capped at TIE_CAP); the truncation is decided on the kernels' side."""
    x, faces, n, counts, clouds, vmask, ref = _grad_reference()
    B = len(counts)
    n_act = int(vmask.sum())
    # the tie points are taken out of the scans themselves (both sides then see the same, shorter, clouds)
    share = sum(int(r[3].sum()) for r in ref) / float(sum(counts))
    print("surface gradient: %.3f %% of the points left out by the medial-axis rule" % (100 * share))
    assert share <= R.TIE_CAP
    kept = [np.nonzero(~r[3])[0] for r in ref]
    sb = scan.ScanBatch([clouds[b][kept[b]] for b in range(B)], DEV)
    trunc = float(np.sqrt(np.median(ref[0][1]))) if truncate else None
    tau2 = float(np.float32(trunc ** 2)) if truncate else np.inf
    ft = scan.FaceTable(faces, n, DEV)
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    matches = {}
    L = scan.chamfer(xd, sb, vertex_mask=vmask, trunc=trunc, w_model_to_scan=w, faces=ft, matches=matches)
    gL = torch.from_numpy(np.random.RandomState(2).randn(B).astype(np.float32)).to(DEV)
    g, = torch.autograd.grad(L, xd, gL)
    gn, gLn, Lh = g.cpu().numpy(), gL.cpu().numpy().astype(np.float64), L.detach().cpu().numpy()
    d2_gpu = matches["d2_surface"].cpu().numpy()
    i_ms, d_ms = (t.cpu().numpy() for t in scan.nearest(xd.detach(), sb.points, t_count=sb.counts))
    assert {"idx_sm", "d2_sm", "face", "uv"} <= set(matches) and tuple(matches["uv"].shape) == (B, sb.points.shape[1], 2)
    cut = total = 0
    for b in range(B):
        k = kept[b]
        m = k.size
        s = clouds[b][k]
        f64, d64, uv64 = ref[b][0][k], ref[b][1][k], ref[b][2][k]
        keep = d2_gpu[b, :m] < np.float32(tau2)
        cut += int((~keep).sum()); total += m
        val = np.minimum(d64, tau2).mean() + (w * np.minimum(scan_ref.nearest_f64(x[b, :n], s)[1][vmask], tau2).sum() / n_act if w > 0 else 0.0)
        # a foot-point error of delta = 4 * 1.01 * 2^-24 * 0.9 moves a distance of about 0.01 (the noise) by 2 delta / 0.01 = 4.3e-5
        assert abs(float(Lh[b]) - val) <= 1e-4 * val, (b, float(Lh[b]), val)
        g64 = np.zeros((x.shape[1], 3))
        g64[:n] = R.surface_grad_f64(s, x[b, :n], faces, f64, uv64, keep, n, m)
        if w > 0:
            on = np.zeros(x.shape[1], bool)
            on[:n] = vmask & (d_ms[b, :n] < np.float32(tau2))
            kk = np.nonzero(on)[0]
            g64[kk] += w * (2.0 / n_act) * (x[b, kk].astype(np.float64) - s[i_ms[b, kk]].astype(np.float64))
        g64 *= gLn[b]
        err, top = np.abs(gn[b] - g64).max(), np.abs(g64).max()
        print("surface gradient b=%d w=%g trunc=%s: max err %.3g of max|g| %.3g (%.3g)" % (b, w, trunc, err, top, err / top))
        assert err <= R.KERNEL_FACTOR * R.F32_GRAD_REL * top, (b, err, top)
        assert float(np.abs(gn[b, n:]).max()) == 0.0 and float(np.abs(gn[b, :n][~vmask]).max()) == 0.0
    if truncate:
        assert 0.2 <= cut / total <= 0.8, (cut, total)


# ------------------------------------------------------------------------------------------------ 6. the old path when off
def test_without_faces_the_vertex_kernels_run_bit_for_bit_and_no_surface_kernel():
    x, faces, n, counts, clouds, vmask = R.case_inputs("template6890.npz", 3, 1000, True, "s01")
    sb = scan.ScanBatch(clouds, DEV)
    for w, trunc in ((0.0, None), (0.5, 0.03)):
        xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
        L = scan.chamfer(xd, sb, vertex_mask=vmask, trunc=trunc, w_model_to_scan=w)
        gL = torch.from_numpy(np.random.RandomState(1).randn(3).astype(np.float32)).to(DEV)
        g, = torch.autograd.grad(L, xd, gL)
        xs = xd.detach()
        tau2 = float("inf") if trunc is None else float(trunc) ** 2
        vm, vsb = ops._mask_arg(vmask, 3, n, xs.device)
        i_sm, d_sm = ops.nearest_points(sb.points, xs, q_count=sb.counts, t_mask=vm, nt=n)
        i_ms, d_ms = ops.nearest_points(xs, sb.points, t_count=sb.counts) if w > 0 else (None, None)
        L0, c0 = ops.chamfer_fwd(d_sm, sb.counts, d_ms, n + 1, n, vm, vsb, tau2, w)
        g0 = ops.chamfer_bwd(xs, n, sb.points, sb.counts, i_sm, d_sm, i_ms, d_ms, vm, vsb, c0, tau2, w, gL)
        assert torch.equal(bits(L.detach()), bits(L0)) and torch.equal(bits(g), bits(g0))
    m, z0, z_kps, dummy, scans, _, nv = semantic_setup()
    h = load_hierarchy(os.path.join(GOLD, "semantic.npz"))
    _lib.profile_enable(True)
    editing.fit_scan(m, z0, z_kps, scans, parts=PARTS, steps=3, lr=1e-2, w_model_to_scan=0.5, dummy=dummy)
    torch.cuda.synchronize()
    names = {k for k, _, _ in _lib.profile_records_by_kernel()}
    _lib.profile_enable(False)
    assert not (names & SURFACE_KERNELS) and {"nearest_search_kernel", "chamfer_bwd_kernel"} <= names, sorted(names)
    _lib.profile_enable(True)
    editing.fit_scan(m, z0, z_kps, scans, parts=PARTS, steps=3, lr=1e-2, w_model_to_scan=0.5, dummy=dummy, faces=h.faces)
    torch.cuda.synchronize()
    names = {k for k, _, _ in _lib.profile_records_by_kernel()}
    _lib.profile_enable(False)
    assert SURFACE_KERNELS <= names and "chamfer_bwd_kernel" not in names, sorted(names)
    assert not [k for k in names if k.startswith("wgrad") or "bwd_wgt" in k or "slab_reduce" in k], sorted(names)


# ------------------------------------------------------------------------------------------------ 7. what it buys
def _surface_rms(scan_clouds, x_fit, faces, n):
    return float(np.sqrt(np.mean([R.closest_f64(s, x_fit[b, :n], faces)[1].mean() for b, s in enumerate(scan_clouds)])))


def test_surface_fit_is_closer_to_surface_sampled_scans_and_no_worse_on_the_vertices():
    """semantic_setup's bodies, scans sampled on the SURFACE of the decoded targets (area-weighted, seeded, 20 000 points, no
    noise), fitted from the same 1.3x start with and without faces (same steps, same rate).  Float64 point-to-surface RMS from
    scan to fitted mesh: lower with faces.  Mean vertex distance to the target: at most 1.10 times the vertex-mode fit's."""
    m, z0, z_kps, dummy, _, x_star, n = semantic_setup()
    faces = np.asarray(load_hierarchy(os.path.join(GOLD, "semantic.npz")).faces, np.int64)
    xs = x_star.cpu().numpy()
    clouds = [R.sample_surface(xs[b, :n], faces, 20000, seed=50 + b) for b in range(3)]
    scans = scan.ScanBatch(clouds, DEV, order="morton")
    ft = scan.FaceTable(faces, n, DEV)
    steps, lr = 400, 2e-3
    zv, _, lv = editing.fit_scan(m, z0, z_kps, scans, parts=PARTS, steps=steps, lr=lr, dummy=dummy)
    zs, _, ls = editing.fit_scan(m, z0, z_kps, scans, parts=PARTS, steps=steps, lr=lr, dummy=dummy, faces=ft)
    with torch.no_grad():
        xv, xf = m.decode(zv, z_kps, dummy), m.decode(zs, z_kps, dummy)
        dist_v = (xv[:, :n] - x_star[:, :n]).norm(dim=2).mean().item()
        dist_s = (xf[:, :n] - x_star[:, :n]).norm(dim=2).mean().item()
    rms_v = _surface_rms(clouds, xv.cpu().numpy(), faces, n)
    rms_s = _surface_rms(clouds, xf.cpu().numpy(), faces, n)
    print("surface-sampled scans: point-to-surface RMS %.5g with faces, %.5g without; mean vertex distance to the target %.5g with, "
          "%.5g without (ratio %.4f); loss %.4g -> %.4g with, %.4g -> %.4g without"
          % (rms_s, rms_v, dist_s, dist_v, dist_s / dist_v, float(ls[0]), float(ls[-1]), float(lv[0]), float(lv[-1])))
    assert float(ls[-1]) < float(ls[0])
    assert rms_s < rms_v, (rms_s, rms_v)
    assert dist_s <= 1.10 * dist_v, (dist_s, dist_v)
    # batched and single-body fits agree bitwise
    zb, fb, lb = editing.fit_scan(m, z0, z_kps, scans, parts=PARTS, steps=30, lr=1e-2, dummy=dummy, faces=ft)
    for b in (0, 2):
        s = slice(b, b + 1)
        z1, f1, _ = editing.fit_scan(m, z0[s], z_kps[s], scans.select(s), parts=PARTS, steps=30, lr=1e-2, dummy=dummy[s], faces=ft)
        assert torch.equal(bits(z1), bits(zb[s])) and torch.equal(bits(f1), bits(fb[s])), b


# ------------------------------------------------------------------------------------------------ 8. at size
@pytest.mark.parametrize("f32_mma", ["planes3"], indirect=True)
def test_surface_fit_at_size(f32_mma):
    """20 steps on the 6890-vertex plain autoencoder, 16 bodies against 50 000-point surface scans: what tools/bench_surface.py times."""
    dev = torch.device(DEV)
    h = load_hierarchy(os.path.join(GOLD, "template6890.npz"))
    torch.manual_seed(5)
    m = sh.SpiralAutoencoder([[3, 16, 32, 64, 128], [[], [], [], [], []]], [[128, 64, 32, 32, 16], [[], [], [], [], 3]], 256, h.sizes,
                             h.spiral_sizes, h.spirals, h.D, h.U, dev)
    B, M = 16, 50000
    x = torch.from_numpy(synthetic.synth_batch(h.verts, B, seed=3)).to(dev)
    with torch.no_grad():
        z_star = m.encode(x)
        x_star = m.decode(z_star)
    n = x_star.shape[1] - 1
    xs = x_star.cpu().numpy()
    faces = np.asarray(h.faces, np.int64)
    scans = scan.ScanBatch([R.sample_surface(xs[b, :n], faces, M, seed=b) for b in range(B)], dev, order="morton")
    before = snapshot(m)
    z0 = z_star * 1.3
    z1, final, losses = editing.fit_scan(m, z0, None, scans, steps=20, lr=1e-2, w_model_to_scan=0.5, faces=scan.FaceTable(faces, n, dev))
    l = losses.cpu()
    print("surface fit at size: loss %.5g -> %.5g" % (float(l[0]), float(l[-1])))
    assert torch.isfinite(l).all() and torch.isfinite(final).all() and float(l[-1]) < float(l[0]), (float(l[0]), float(l[-1]))
    assert z1.shape == z0.shape and not torch.equal(z1, z0)
    for k, p in m.named_parameters():
        assert torch.equal(p.detach(), before[k]) and p.requires_grad and p.grad is None, k
