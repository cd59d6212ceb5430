"""Point-to-surface alignment on the GPU: the surface moments against float64, the closed form on surface pairs, descent and
recovery of scan.align(faces=), determinism and batching, editing.register_scan(align_on="surface"), and the argument errors."""
import functools
import os

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, editing, ops, scan
from semantichuman_amd.hierarchy import load_hierarchy
from tests import align_ref as A
from tests import align_surface_ref as AS
from tests import scan_ref
from tests import surface_ref as S
from tests.launch_record import launch_counts as launches
from tests.test_align import MODES, MOVES, PARTS, check_rotation, ragged_counts, semantic_setup

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
U24, U53 = 2.0 ** -24, 2.0 ** -53
RANGE = 2048                                                               # SH_ALIGN_RANGE
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1.0])


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return torch.equal(bits(a.contiguous()), bits(b.contiguous()))


@functools.lru_cache(maxsize=None)
def mesh(name):
    h = load_hierarchy(os.path.join(GOLD, name))
    return np.asarray(h.verts, np.float64), np.asarray(h.faces, np.int64)


def surface_searches(sb, xd, n, ft, vmask, w):
    """What a forward pass records: (face, d2_surface, uv, idx_ms, d2_ms)."""
    _, d_v = ops.nearest_points(sb.points, xd, q_count=sb.counts, t_mask=vmask, nt=n)
    face, d2, uv = ops.nearest_surface(sb.points, xd, ft.faces, n, sb.counts, vmask, d_v)
    i_ms, d_ms = ops.nearest_points(xd, sb.points, t_count=sb.counts) if w > 0 else (None, None)
    return face, d2, uv, i_ms, d_ms


def gpu_moments(sb, xd, n, vmask, ft, m, tau2, w, mode="similarity", pose=None):
    """(mom [B, 20] float64, inc [B, 13], pose_out [B, 12], scale_out [B]) from the surface matches m of surface_searches."""
    B = xd.shape[0]
    vm, vsb = ops._mask_arg(vmask, B, n, xd.device)
    part = ops.align_moments_surface(sb.points, sb.counts, xd, n, vm, vsb, ft.faces, m[0], m[2], m[1], m[3], m[4], tau2, w)
    assert not torch.isnan(part).any()
    mom = torch.full((B, 20), float("nan"), dtype=torch.float64, device=DEV)
    inc = torch.full((B, 13), float("nan"), device=DEV)
    pose = scan.Pose.identity(B, DEV) if pose is None else pose
    out, sc = torch.full((B, 12), float("nan"), device=DEV), torch.full((B,), float("nan"), device=DEV)
    ops.align_solve(part, sb.points.shape[1], n, sb.counts, w, mode, pose.packed, pose.scale, out, sc, inc, mom)
    return mom.cpu().numpy(), inc.cpu().numpy().astype(np.float64), out.cpu().numpy(), sc.cpu().numpy()


def host(m):
    return [None if t is None else t.cpu().numpy() for t in m]


# ------------------------------------------------------------------------------------------------ 1. moments against float64
@pytest.mark.parametrize("B,M", [(B, M) for M in (1, 63, 1000, 20011) for B in (1, 3, 16)] + [(3, RANGE + 1)])
def test_surface_moments_against_float64(B, M):
    x, faces, n, counts, clouds, _ = S.case_inputs("template6890.npz", B, M, False, "s0")      # samples of a neighbour body's surface
    assert counts == ragged_counts(B, M)
    sb = scan.ScanBatch(clouds, DEV)
    xd = torch.from_numpy(x).to(DEV)
    ft = scan.FaceTable(faces, n, DEV)
    rs = np.random.RandomState(7)
    worst = 0.0
    for masked in (False, True):
        vmask = rs.rand(n) < 0.7 if masked else None
        for w in (0.0, 0.5):
            m = surface_searches(sb, xd, n, ft, vmask, w)
            mh = host(m)
            for truncate in (False, True):
                tau2 = float(np.float32(np.median(mh[1][0, :counts[0]]))) if truncate else float("inf")
                mom, _, _, _ = gpu_moments(sb, xd, n, vmask, ft, m, tau2, w)
                for b in range(B):
                    p, q, wt = AS.pairs_surface(clouds[b], x[b], n, counts[b], vmask, faces, mh[0][b], mh[2][b], mh[1][b],
                                                None if mh[3] is None else mh[3][b], None if mh[4] is None else mh[4][b], tau2, w)
                    ref, mag = A.moments(p, q, wt)
                    K = len(wt)
                    assert mom[b, 18] == K and mom[b, 19] == 0.0, (b, mom[b, 18], K)               # the kept count is exact
                    # Derived.  With contraction off the kernel's q is numpy's q bit for bit, so both sides add the same terms.
                    # A product of two fp32 values is exact in fp64; a product with a coordinate of q (53 bits) is rounded once, or
                    # fused into the running sum and not rounded at all: at most 2^-53 |term| on either side, and |q|^2 (three such
                    # products, two additions of positive numbers) at most 3 x 2^-53 |term|.  The order of a K-term fp64 sum adds
                    # (K - 1) 2^-53 sum|term| for either order, and the weight and the three-term |p|^2 a few roundings, as in
                    # test_align.test_moments_against_float64 (its 16).  Bound: 2 (K + 16 + 4) 2^-53 sum w|term|.
                    bound = 2 * (K + 16 + 4) * U53 * mag[:18]
                    err = np.abs(mom[b, :18] - ref[:18])
                    worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                    assert (err <= bound).all(), (b, masked, w, truncate, err, bound)
    print("surface moments B=%d M=%d: largest error / bound %.3g" % (B, M, worst))


def test_a_body_with_every_vertex_masked_keeps_no_pair():
    x, faces, n, counts, clouds, _ = S.case_inputs("template6890.npz", 2, 1000, False, "s0")
    sb = scan.ScanBatch(clouds, DEV)
    xd = torch.from_numpy(x).to(DEV)
    ft = scan.FaceTable(faces, n, DEV)
    vmask = np.ones((2, n), bool)
    vmask[1] = False
    for w in (0.0, 0.5):
        m = surface_searches(sb, xd, n, ft, vmask, w)
        assert (m[0][1] == -1).all() and (m[0][0, :counts[0]] >= 0).all()
        mom, inc, out, sc = gpu_moments(sb, xd, n, vmask, ft, m, float("inf"), w)
        assert mom[1, 18] == 0 and mom[1, 0] == 0 and np.array_equal(inc[1], IDENTITY), (mom[1], inc[1])
        assert np.array_equal(out[1], IDENTITY[:12].astype(np.float32)) and sc[1] == 1.0
        assert mom[0, 18] == counts[0] + (n if w > 0 else 0) and not np.array_equal(inc[0], IDENTITY)


def test_surface_form_at_a_corner_is_the_vertex_form_bit_for_bit():
    """The two partner forms run one walk.  A foot point with uv = 0 on a face whose corner 0 is the recorded nearest vertex is
    (double)a + (0 ab + 0 ac) = a exactly, so the surface form must return the vertex form's partial sums and pose, byte for byte."""
    v, faces = mesh("small_ae.npz")
    n, B, M = v.shape[0], 2, 300
    x = scan_ref.model_points(v, B, seed=3)
    clouds = [S.sample_surface(x[(b + 1) % B, :n], faces, m, seed=50 + b, sigma=0.01) for b, m in enumerate((300, 17))]
    sb = scan.ScanBatch(clouds, DEV)
    xd = torch.from_numpy(x).to(DEV)
    # a copy of the face table in which every vertex is corner 0 of a face of its own: rows rotated, none used twice
    table, own, used = faces.copy(), np.full(n, -1), np.zeros(len(faces), bool)
    for i in range(n):
        k = int(np.nonzero((faces == i).any(1) & ~used)[0][0])
        table[k], own[i], used[k] = np.roll(faces[k], -int(np.nonzero(faces[k] == i)[0][0])), k, True
    assert (table[own, 0] == np.arange(n)).all()
    ft = scan.FaceTable(table, n, DEV)
    idx, d_v = ops.nearest_points(sb.points, xd, q_count=sb.counts, nt=n)
    ih = idx.cpu().numpy()
    assert ((ih[0] >= 0) & (ih[0] < n)).all() and ((ih[1, :17] >= 0) & (ih[1, :17] < n)).all()
    face = torch.from_numpy(np.where(ih >= 0, own[np.clip(ih, 0, n - 1)], -1).astype(np.int32)).to(DEV)
    uv = torch.zeros((B, M, 2), device=DEV)
    tau2 = float(np.float32(np.median(d_v[0].cpu().numpy())))                  # drops half of body 0's pairs
    vm, vsb = ops._mask_arg(None, B, n, xd.device)
    for w in (0.0, 0.5):
        i_ms, d_ms = ops.nearest_points(xd, sb.points, t_count=sb.counts) if w > 0 else (None, None)
        pv = ops.align_moments(sb.points, sb.counts, xd, n, vm, vsb, idx, d_v, i_ms, d_ms, tau2, w)
        ps = ops.align_moments_surface(sb.points, sb.counts, xd, n, vm, vsb, ft.faces, face, uv, d_v, i_ms, d_ms, tau2, w)
        kept = pv[:, 0, 0].cpu().numpy()
        assert 0 < kept[0] < 300 and kept[1] <= 17, kept
        assert same(pv, ps), (w, (pv != ps).nonzero().cpu().numpy())
        poses = []
        for part in (pv, ps):
            out, sc = torch.full((B, 12), float("nan"), device=DEV), torch.full((B,), float("nan"), device=DEV)
            pose = scan.Pose.identity(B, DEV)
            ops.align_solve(part, M, n, sb.counts, w, "similarity", pose.packed, pose.scale, out, sc)
            poses.append((out, sc))
        assert torch.isfinite(poses[0][0]).all() and same(poses[0][0], poses[1][0]) and same(poses[0][1], poses[1][1]), w


# ------------------------------------------------------------------------------------------------ 2. solve on surface pairs
@pytest.mark.parametrize("mode", MODES)
def test_solve_on_surface_pairs_against_umeyama(mode):
    v, faces = mesh("template6890.npz")
    n = v.shape[0]
    B = 4
    x = scan_ref.model_points(v, B, seed=3)
    clouds = [AS.moved_surface_scan(x[b, :n], faces, case, m=3000 + 7 * b, seed=40 + b)[0] for b, case in enumerate(A.SIMILARITY_CASES)]
    sb = scan.ScanBatch(clouds, DEV)
    xd = torch.from_numpy(x).to(DEV)
    ft = scan.FaceTable(faces, n, DEV)
    w = 0.5
    m = surface_searches(sb, xd, n, ft, None, w)
    mh = host(m)
    mom, inc, _, _ = gpu_moments(sb, xd, n, None, ft, m, float("inf"), w, mode)
    for b in range(B):
        Rg, c = check_rotation(inc[b])
        Ar, tr, cr, Rr = A.umeyama(mom[b], mode)
        p = clouds[b].astype(np.float64)
        got, ref = A.apply(inc[b, :9].reshape(3, 3), inc[b, 9:12], p), A.apply(Ar, tr, p)
        extent = max(np.abs(ref).max(), np.abs(p).max())
        # test_align.test_solve_against_umeyama's tolerance: the increment is the float64 solution rounded to fp32 entry by entry
        # (three products and a translation, each off by at most 2^-24 of its size -> 4 x 2^-24 x extent; Jacobi against SVD ~1e-15): 8 x.
        assert np.abs(got - ref).max() <= 8 * U24 * extent, (mode, b)
        if mode != "similarity":
            assert inc[b, 12] == 1.0
        if mode == "translation":
            assert np.array_equal(inc[b, :9].reshape(3, 3), np.eye(3))
        pp, qq, wt = AS.pairs_surface(clouds[b], x[b], n, len(clouds[b]), None, faces, mh[0][b], mh[2][b], mh[1][b], mh[3][b], mh[4][b],
                                      float("inf"), w)
        before = A.residual(pp, qq, wt, np.eye(3), np.zeros(3))
        after = A.residual(pp, qq, wt, inc[b, :9].reshape(3, 3), inc[b, 9:12])
        print("surface solve %s b=%d: |dp| %.3g (bound %.3g), c %.6f vs %.6f, residual %.6g -> %.6g"
              % (mode, b, np.abs(got - ref).max(), 8 * U24 * extent, c, cr, before, after))
        assert after <= before, (mode, b, before, after)


# ------------------------------------------------------------------------------------------------ shared moved surface scans
@functools.lru_cache(maxsize=None)
def moved_surface_batch(template, ncases, m):
    v, faces = mesh(template)
    n = v.shape[0]
    x = scan_ref.model_points(v, 4, seed=3)
    moved = [AS.moved_surface_scan(x[k, :n], faces, case, m=m, seed=100 + k) for k, case in enumerate(A.SIMILARITY_CASES[:ncases])]
    return x, faces, n, moved


# ------------------------------------------------------------------------------------------------ 3. descent
@pytest.mark.parametrize("truncate", [False, True])
@pytest.mark.parametrize("w", [0.0, 1.0])
@pytest.mark.parametrize("mode", MODES)
def test_surface_align_never_raises_the_surface_chamfer_value(mode, w, truncate):
    x, faces, n, moved = moved_surface_batch("template6890.npz", 3, 5000)
    xd = torch.from_numpy(x[:3]).to(DEV)
    sb = scan.ScanBatch([mv[0] for mv in moved], DEV)
    trunc = 0.05 if truncate else None
    pose, aligned, log = scan.align(xd, sb, mode=mode, iters=15, w_model_to_scan=w, trunc=trunc, faces=faces)
    L = log.cpu().numpy().astype(np.float64)
    assert L.shape == (15, 3) and np.isfinite(L).all()
    # test_align.test_align_never_raises_the_chamfer_value's derivation, which does not depend on what the partner is.  Fixed
    # matches, then least squares over the pose, then re-matching: no term of the (truncated) loss can rise - in exact arithmetic.
    # The transformed points are stored in fp32 (each coordinate off by up to d = 4 x 2^-24 x extent: three products and the
    # translation), which changes a squared distance by up to 2 d sqrt(d2) and so the mean by up to 2 d sqrt(L) (Cauchy-Schwarz),
    # on either side of the comparison; the fp32 rounding of the logged value itself is 2^-24 L.
    extent = float(np.abs(x).max()) * 1.5
    tol = 2 * (2 * 4 * U24 * extent * np.sqrt((1 + w) * L[:-1])) + 2 * U24 * L[:-1]
    rise = L[1:] - L[:-1]
    print("surface descent %s w=%g trunc=%s: %s -> %s, largest rise / tolerance %.3g" % (mode, w, trunc, L[0], L[-1], float((rise / tol).max())))
    assert (rise <= tol).all(), (rise / tol).max()
    assert (L[-1] < L[0]).all()


# ------------------------------------------------------------------------------------------------ 4. recovery
@functools.lru_cache(maxsize=None)
def recovery_runs():
    """Both GPU loops on the four moved scans of the CPU study, once: (pose with faces, pose without)."""
    x, faces, n, moved = AS.study_inputs()
    xd = torch.from_numpy(x).to(DEV)
    sb = scan.ScanBatch([mv[0] for mv in moved], DEV)
    ps, _, _ = scan.align(xd, sb, mode="similarity", iters=40, w_model_to_scan=0.0, faces=faces)
    pv, _, _ = scan.align(xd, sb, mode="similarity", iters=40, w_model_to_scan=0.0)
    return x, faces, n, moved, ps, pv


@pytest.mark.parametrize("k", range(4))
def test_surface_align_recovers_scale_and_pose(k):
    x, faces, n, moved, ps, pv = recovery_runs()
    s, pts, (At, tt), extent = moved[k]
    xb = x[k, :n].astype(np.float64)
    As_, ts_ = ps.A[k].double().cpu().numpy(), ps.t[k].double().cpu().numpy()
    Av_, tv_ = pv.A[k].double().cpu().numpy(), pv.t[k].double().cpu().numpy()
    c_true = AS.scale_of(At)
    rel = abs(float(ps.scale[k]) / c_true - 1)
    e_s, e_v = AS.pose_error(As_, ts_, s, pts), AS.pose_error(Av_, tv_, s, pts)
    Ar, tr, _ = AS.icp_surface(xb, faces, s, "similarity", 40, "moments", 0.0)
    r_gpu = AS.surface_rms(A.apply(As_, ts_, s.astype(np.float64)), xb, faces)
    r_ref = AS.surface_rms(A.apply(Ar, tr, s.astype(np.float64)), xb, faces)
    print("surface recovery %s: scale %.6f (true %.4f, error %.3g; vertex align %.6f), pose error %.3g of the extent (vertex align %.3g, "
          "ratio %.3g), surface RMS %.4g against float64 surface ICP %.4g (x %.4f)"
          % (A.SIMILARITY_CASES[k], float(ps.scale[k]), c_true, rel, float(pv.scale[k]), e_s / extent, e_v / extent, e_s / e_v, r_gpu, r_ref,
             r_gpu / r_ref))
    assert rel <= 1e-3, rel
    assert e_s <= 0.25 * e_v, (e_s, e_v)
    # 1.05: what test_align.test_align_recovers_the_moved_scans gives a kernel loop over its float64 loop; the additive term is the
    # fp32 storage of the transformed points (8 x 2^-24 x extent)
    assert r_gpu <= 1.05 * r_ref + 8 * U24 * extent, (r_gpu, r_ref)


# ------------------------------------------------------------------------------------------------ 5. determinism and batching
def test_surface_align_is_deterministic_batch_chunk_and_cull_independent():
    v, faces = mesh("template6890.npz")
    n = v.shape[0]
    B = 16
    x = scan_ref.model_points(v, B, seed=3)
    counts = ragged_counts(B, 20011)
    clouds = [AS.moved_surface_scan(x[b, :n], faces, A.SIMILARITY_CASES[b % 3], m=counts[b], seed=7 + b)[0] for b in range(B)]
    xd = torch.from_numpy(x).to(DEV)
    sb = scan.ScanBatch(clouds, DEV)
    ft = scan.FaceTable(faces, n, DEV)
    kw = dict(mode="similarity", iters=8, w_model_to_scan=1.0, trunc=0.2, faces=ft)
    p1, a1, l1 = scan.align(xd, sb, **kw)
    p2, a2, l2 = scan.align(xd, sb, **kw)
    assert same(p1.packed, p2.packed) and same(p1.scale, p2.scale) and same(l1, l2) and same(a1.points, a2.points)
    assert torch.isfinite(l1).all() and torch.isfinite(p1.packed).all()
    for b in (0, 5, 11, 15):
        ps, as_, ls = scan.align(xd[b:b + 1], scan.ScanBatch([clouds[b]], DEV), **kw)       # alone, and with M = its own count
        assert same(ps.packed[0], p1.packed[b]) and same(ps.scale[0], p1.scale[b]), b
        assert same(ls[:, 0], l1[:, b]), b
        assert same(as_.points[0], a1.points[b, :counts[b]]), b
    for chunks in (1, 3, 7):
        pc, _, lc = scan.align(xd[:2], sb.select(slice(0, 2)), chunks=chunks, **kw)
        assert same(pc.packed, p1.packed[:2]) and same(lc, l1[:, :2]), chunks
    small = scan.ScanBatch([clouds[0][:1000], clouds[1][:1000]], DEV)                        # the unculled sweep is slow: two bodies, M = 1000
    pa, aa, la = scan.align(xd[:2], small, cull=True, **kw)
    pb, ab, lb = scan.align(xd[:2], small, cull=False, **kw)
    assert same(pa.packed, pb.packed) and same(pa.scale, pb.scale) and same(la, lb) and same(aa.points, ab.points)


# ------------------------------------------------------------------------------------------------ 6. register_scan
@functools.lru_cache(maxsize=None)
def register_setup():
    """test_align.semantic_setup's model and 1.3x start; scans = 5000 samples of each decoded target's SURFACE, carried into a
    frame of their own by the inverse of MOVES."""
    m, z0, z_kps, dummy, _, x_star, n = semantic_setup()
    faces = np.asarray(load_hierarchy(os.path.join(GOLD, "semantic.npz")).faces, np.int64)
    xs = x_star.cpu().numpy()
    truth, clouds = [], []
    for b in range(3):
        pts = S.sample_surface(xs[b, :n], faces, 5000, seed=50 + b).astype(np.float64)
        At, tt = A.true_pose(MOVES[b % 3], float((pts.max(0) - pts.min(0)).max()))
        clouds.append(A.apply(*A.inverse(At, tt), pts).astype(np.float32))
        truth.append((pts, At))
    return m, z0, z_kps, dummy, clouds, truth, x_star, n, faces, scan.FaceTable(faces, n, DEV)


def test_register_scan_on_the_surface():
    m, z0, z_kps, dummy, clouds, truth, x_star, n, faces, ft = register_setup()
    sb = scan.ScanBatch(clouds, DEV)
    kw = dict(parts=PARTS, steps=60, lr=2e-3, dummy=dummy, faces=ft, align_iters=15)
    zs, pose_s, fs, ls = editing.register_scan(m, z0, z_kps, sb, align_on="surface", **kw)
    zv, pose_v, fv, lv = editing.register_scan(m, z0, z_kps, sb, align_on="vertices", **kw)
    zd, pose_d, fd, ld = editing.register_scan(m, z0, z_kps, sb, **kw)
    l = ls.cpu()
    assert torch.isfinite(l).all() and torch.isfinite(fs).all() and float(l[-1]) < float(l[0]), (float(l[0]), float(l[-1]))
    # "vertices" is the code path of a call without the argument, bit for bit
    assert same(zv, zd) and same(pose_v.packed, pose_d.packed) and same(pose_v.scale, pose_d.scale) and same(fv, fd) and same(lv, ld)
    assert not same(pose_s.packed, pose_v.packed)
    for name, pose, final in (("surface", pose_s, fs), ("vertices", pose_v, fv)):          # recorded, not gated
        err = [AS.pose_error(pose.A[b].double().cpu().numpy(), pose.t[b].double().cpu().numpy(), clouds[b], truth[b][0])
               / float((truth[b][0].max(0) - truth[b][0].min(0)).max()) for b in range(3)]
        sc = [float(pose.scale[b]) / AS.scale_of(truth[b][1]) - 1 for b in range(3)]
        print("register_scan align_on=%s: final surface Chamfer %s, pose error / extent %s, scale error %s"
              % (name, final.cpu().numpy(), np.array(err), np.array(sc)))
    # a batched run equals the single-body runs, bitwise
    for b in range(3):
        s = slice(b, b + 1)
        z1, p1, f1, l1 = editing.register_scan(m, z0[s], z_kps[s], sb.select(s), align_on="surface", **dict(kw, dummy=dummy[s]))
        assert same(z1, zs[s]) and same(p1.packed, pose_s.packed[s]) and same(p1.scale, pose_s.scale[s]) and same(f1, fs[s]), b


def test_register_scan_surface_step_launches_three_kernels_and_no_search():
    m, z0, z_kps, dummy, clouds, truth, x_star, n, faces, ft = register_setup()
    sb = scan.ScanBatch(clouds, DEV)
    unmoved = scan.ScanBatch([t[0].astype(np.float32) for t in truth], DEV)
    kw = dict(parts=PARTS, steps=5, lr=1e-2, w_model_to_scan=0.5, dummy=dummy, faces=ft)
    _, n_fit = launches(lambda: editing.fit_scan(m, z0, z_kps, unmoved, **kw))
    r, n_reg = launches(lambda: editing.register_scan(m, z0, z_kps, sb, align_iters=0, align_every=1, align_on="surface", **kw))
    print("fit_scan launches %s\nregister_scan launches %s" % (sorted(n_fit.items()), sorted(n_reg.items())))
    # 5 steps and the final evaluation search in both functions; the 5 pose updates add no search of either kind
    for k in ("nearest_search_kernel", "surface_search_kernel", "surface_prep_kernel", "surface_finish_kernel"):
        assert n_reg[k] == n_fit[k], (k, n_reg[k], n_fit[k])
    assert n_reg["nearest_search_kernel"] == 12
    assert n_reg["align_moments_surface_kernel"] == 5 and n_reg["align_solve_kernel"] == 5 and "align_moments_kernel" not in n_reg
    assert n_reg["transform_points_kernel"] == 5 + 1                       # + the start pose applied once
    assert not [k for k in n_fit if k.startswith(("align_", "transform_points"))]
    r2 = editing.register_scan(m, z0, z_kps, sb, align_iters=0, align_every=1, align_on="surface", **kw)
    assert same(r[0], r2[0]) and same(r[1].packed, r2[1].packed) and same(r[3], r2[3])


# ------------------------------------------------------------------------------------------------ 7. errors
def test_argument_errors():
    x, faces, n, counts, clouds, _ = S.case_inputs("small_ae.npz", 2, 63, False, "s0")
    xd = torch.from_numpy(x).to(DEV)
    sb = scan.ScanBatch(clouds, DEV)
    z = torch.zeros((2, 17, 8), device=DEV)
    with pytest.raises(ValueError, match="faces"):
        editing.register_scan(None, z, z, sb, align_on="surface")
    matches = {}
    scan.chamfer(xd, sb, matches=matches)                                  # a vertex forward pass: no face, no uv
    with pytest.raises(ValueError, match="surface"):
        scan.pose_update(scan.Pose.identity(2, DEV), sb, scan.Pose.identity(2, DEV).apply(sb), matches, surface=True)
    normals = [np.tile(np.array([[0.0, 0.0, 1.0]]), (c, 1)) for c in counts]
    with pytest.raises(ValueError, match="not built"):
        scan.align(xd, scan.ScanBatch(clouds, DEV, normals=normals), faces=faces, normal_angle=60.0, normal_faces=faces, trunc=0.1)
    with pytest.raises(ValueError, match="face table made for"):
        scan.align(xd, sb, faces=scan.FaceTable(faces, n + 1, DEV))
    matches = {}
    scan.chamfer(xd, sb, matches=matches, faces=faces)                     # and a surface pass records what the update needs
    assert {"face", "uv", "d2_surface", "faces"} <= set(matches)
    pose, al = scan.Pose.identity(2, DEV), scan.Pose.identity(2, DEV).apply(sb)
    scan.pose_update(pose, sb, al, matches, surface=True)
    assert torch.isfinite(pose.packed).all()
