"""The point-to-plane pose step on the GPU: both moments kernels against float64 sums over the GPU's own matches, the solve against
the reference's solve of the GPU's own system, the singular rules, determinism and batching, recovery on the study cases, the
vertex form, editing.register_scan(align_step="plane"), and "off means off"."""
import functools
import os

import numpy as np
import pytest
import torch

import semantichuman_amd as sh
from semantichuman_amd import editing, ops, scan
from semantichuman_amd.hierarchy import load_hierarchy
from tests import align_ref as A
from tests import align_plane_ref as AP
from tests import align_surface_ref as AS
from tests import scan_ref
from tests import surface_ref as S
from tests.test_align import MODES, MOVES, final_rms, searches
from tests.test_align_surface import host, mesh, same, surface_searches

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
U24, U53 = 2.0 ** -24, 2.0 ** -53


def plane_system_gpu(sb, xd, n, vmask, ft, tn, m, tau2, w, surface, mode="similarity", pose=None):
    """(sys [B, 37] float64, kept pairs [B], pose_out [B, 12], scale_out [B], solved [B]) from the matches m: surface_searches'
    tuple (surface form) or test_align.searches' (vertex form)."""
    B = xd.shape[0]
    vm, vsb = ops._mask_arg(vmask, B, n, xd.device)
    if surface:
        part = ops.align_plane_moments_surface(sb.points, sb.counts, xd, n, vm, vsb, tn if w > 0 else None, ft.faces, m[0], m[2], m[1], m[3], m[4],
                                               tau2, w)
    else:
        part = ops.align_plane_moments(sb.points, sb.counts, xd, n, vm, vsb, tn, m[0], m[1], m[2], m[3], tau2, w)
    assert tuple(part.shape[1:]) == (ops._lib.load().sh_align_ranges(sb.points.shape[1], n, w), 38) and not torch.isnan(part).any()
    sys = torch.full((B, 37), float("nan"), dtype=torch.float64, device=DEV)
    pose = scan.Pose.identity(B, DEV) if pose is None else pose
    out, sc = torch.full((B, 12), float("nan"), device=DEV), torch.full((B,), float("nan"), device=DEV)
    solved = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ops.align_plane_solve(part, sb.points.shape[1], n, sb.counts, w, mode, pose.packed, pose.scale, out, sc, sys, solved)
    kept = part[:, :, 0].sum(1)
    return sys.cpu().numpy(), kept.cpu().numpy(), out.cpu().numpy(), sc.cpu().numpy(), solved.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. moments against float64
def moments_case(template, counts, masked, seed=3):
    v, faces = mesh(template)
    n = v.shape[0]
    B = len(counts)
    x = scan_ref.model_points(v, B, seed=seed)
    clouds = [S.sample_surface(x[(b + 1) % B, :n], faces, c, seed=90 + b) for b, c in enumerate(counts)]     # a neighbour body's surface
    vmask = (np.random.RandomState(7).rand(n) < 0.7) if masked else None
    return x, faces, n, clouds, vmask


@pytest.mark.parametrize("template,counts", [("small_ae.npz", (0, 2049, 2125)), ("template6890.npz", (5000, 4999))])
@pytest.mark.parametrize("surface", [False, True])
def test_plane_moments_against_float64(template, counts, surface):
    x, faces, n, clouds, vmask = moments_case(template, counts, masked=template == "small_ae.npz")
    B = len(counts)
    sb = scan.ScanBatch(clouds, DEV)
    assert sb.points.shape[1] == max(counts)
    xd = torch.from_numpy(x).to(DEV)
    ft = scan.FaceTable(faces, n, DEV)
    tn = scan.vertex_normals(xd, ft)
    tnh = tn.cpu().numpy()
    worst = 0.0
    for w in (0.0, 1.0):
        m = surface_searches(sb, xd, n, ft, vmask, w) if surface else searches(sb, xd, n, vmask, w)
        mh = host(m)
        d_first = mh[1][1, :counts[1]]
        tau2 = float(np.float32(np.median(d_first)))                                                         # trunc set: about half the pairs go
        sys, kept, _, _, _ = plane_system_gpu(sb, xd, n, vmask, ft, tn, m, tau2, w, surface)
        for b in range(B):
            if surface:
                p, q, nrm, wt = AP.pairs_plane(clouds[b], x[b], n, counts[b], vmask, None, None, None if mh[3] is None else mh[3][b],
                                               None if mh[4] is None else mh[4][b], tau2, w, tn=tnh[b], surface=(faces, mh[0][b], mh[2][b], mh[1][b]))
            else:
                p, q, nrm, wt = AP.pairs_plane(clouds[b], x[b], n, counts[b], vmask, mh[0][b], mh[1][b], None if mh[2] is None else mh[2][b],
                                               None if mh[3] is None else mh[3][b], tau2, w, tn=tnh[b])
            ref, mag = AP.plane_system(p, q, nrm, wt)
            K = len(wt)
            assert kept[b] == K or (counts[b] == 0 and K == 0), (b, kept[b], K)                                   # the kept count is exact
            # Derived.  With contraction off the kernel forms p - q, r, J and every product J_i J_j, J_i r, r r with the operations
            # numpy uses on the same fp64 inputs (the foot point, the face normal and the widened fp32 values are bit for bit
            # numpy's), so both sides add the same K terms.  A K-term fp64 sum in any order is within (K - 1) 2^-53 sum |term| of
            # the exact one, on either side; the weight (a division and a product per direction) and the joining add a few
            # roundings - the 16 of test_align.test_moments_against_float64.  Bound: 2 (K + 16) 2^-53 sum w |term|.
            bound = 2 * (K + 16) * U53 * mag[:37]
            err = np.abs(sys[b] - ref[:37])
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (b, w, err, bound)
            if counts[b] == 0:
                assert not sys[b].any()
    print("plane moments %s surface=%s: largest error / bound %.3g" % (template, surface, worst))


# ------------------------------------------------------------------------------------------------ 2. solve against plane_solve
@functools.lru_cache(maxsize=None)
def study_batch():
    x, faces, n, moved = AS.study_inputs()
    return x, faces, n, moved, torch.from_numpy(x).to(DEV), scan.ScanBatch([mv[0] for mv in moved], DEV), scan.FaceTable(faces, n, DEV)


@pytest.mark.parametrize("mode", MODES)
def test_plane_solve_against_the_reference_on_its_own_system(mode):
    x, faces, n, moved, xd, sb, ft = study_batch()
    B = 4
    w = 0.5
    start = scan.moment_pose(sb, xd, n, None, scale=True)
    al = start.apply(sb)
    tn = scan.vertex_normals(xd, ft)
    m = surface_searches(al, xd, n, ft, None, w)
    sys, kept, out, sc, solved = plane_system_gpu(al, xd, n, None, ft, tn, m, float("inf"), w, True, mode)
    alh = al.points.cpu().numpy().astype(np.float64)
    for b in range(B):
        cR, t, c, Rm, ok, delta = AP.plane_solve(sys[b], mode)
        assert ok == 1 and solved[b] == 1
        p = alh[b, :len(moved[b][0])]
        got = A.apply(out[b, :9].astype(np.float64).reshape(3, 3), out[b, 9:].astype(np.float64), p)
        ref = A.apply(cR, t, p)
        extent = max(np.abs(ref).max(), np.abs(p).max())
        cond = AP.condition(sys[b], mode)
        # Derived.  The kernel's pose is its float64 solution rounded to fp32 entry by entry: a coordinate of a moved point is three
        # products and the translation, each off by at most 2^-24 of its size <= extent, 4 x 2^-24 x extent; a displacement has three
        # coordinates (sqrt 3).  The float64 solution itself: the normal equations give delta to cond(H_scaled) 2^-53 relative, times
        # a small constant (64, as in the host test against lstsq: the 7 x 7 factorisation, exp / sin / cos to a few ulp), and an
        # error in delta moves a point by at most that times the extent (|delta| < 1).
        bound = np.sqrt(3.0) * 4 * U24 * extent + 64 * cond * U53 * extent
        disp = float(np.sqrt(((got - ref) ** 2).sum(1).max()))
        print("plane solve %s b=%d: displacement %.3g (bound %.3g, share %.3g), cond %.3g, |delta| %.3g"
              % (mode, b, disp, bound, disp / bound, cond, np.abs(delta).max()))
        assert disp <= bound, (mode, b, disp, bound)
        assert abs(sc[b] / np.float32(c) - 1) <= 2 * U24
        if mode != "similarity":
            assert sc[b] == 1.0
        if mode == "translation":
            assert np.array_equal(out[b, :9].reshape(3, 3), np.eye(3, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ 3. singular cases
def start_pose(B):
    Ast = np.stack([1.1 * A.rotation(A.AXIS, 7.0 + b) for b in range(B)])
    tst = np.stack([[0.01 * b, -0.02, 0.03] for b in range(B)])
    return scan.Pose(torch.from_numpy(Ast).float().to(DEV), torch.from_numpy(tst).float().to(DEV), torch.full((B,), 1.1))


@pytest.mark.parametrize("mode", MODES)
def test_singular_bodies_keep_their_pose_and_leave_the_others_alone(mode):
    x, faces, n, moved, xd, sb, ft = study_batch()
    flat = x[3].copy()
    flat[:, 2] = 0.0                                                        # every face normal is (0, 0, +-1): parallel
    xs = torch.from_numpy(np.stack([x[0], x[1], x[2], flat])).to(DEV)
    clouds = [moved[0][0], np.zeros((0, 3), np.float32), moved[2][0][:1], moved[3][0]]   # regular, empty scan, one pair, flat target
    sbs = scan.ScanBatch(clouds, DEV)
    init = start_pose(4)
    kw = dict(mode=mode, iters=3, w_model_to_scan=0.0, faces=ft, step="plane")
    pose, aligned, log = scan.align(xs, sbs, init=init, **kw)
    solved = pose.solved.cpu().numpy()
    assert solved.shape == (3, 4) and (solved[:, 0] == 1).all() and (solved[:, 1:] == 0).all(), solved
    assert same(pose.packed[1:], init.packed[1:]) and same(pose.scale[1:], init.scale[1:])
    assert not same(pose.packed[0], init.packed[0])
    p1, a1, l1 = scan.align(xs[:1], scan.ScanBatch(clouds[:1], DEV), init=init.select(slice(0, 1)), **kw)
    assert same(p1.packed[0], pose.packed[0]) and same(p1.scale[0], pose.scale[0]) and same(l1[:, 0], log[:, 0])
    assert same(p1.solved[:, 0], pose.solved[:, 0])


def test_a_flat_square_target_is_singular_in_rigid_mode():
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    rs = np.random.RandomState(0)
    cloud = np.concatenate([rs.rand(300, 2), 0.05 + 0.01 * rs.rand(300, 1)], 1).astype(np.float32)
    xd = torch.from_numpy(np.stack([sq, sq])).to(DEV)
    sb = scan.ScanBatch([cloud, cloud[:100]], DEV)
    for w in (0.0, 1.0):
        init = start_pose(2)
        before = init.clone()
        pose, _, _ = scan.align(xd, sb, mode="rigid", iters=2, init=init, w_model_to_scan=w, n=4, faces=faces, step="plane")
        assert (pose.solved.cpu().numpy() == 0).all()
        assert same(pose.packed, before.packed) and same(pose.scale, before.scale)
    # even a translation is singular there: the two in-plane unknowns have no equation
    pose, _, _ = scan.align(xd, sb, mode="translation", iters=1, init=start_pose(2), w_model_to_scan=0.0, n=4, faces=faces, step="plane")
    assert (pose.solved.cpu().numpy() == 0).all()


# ------------------------------------------------------------------------------------------------ 4. determinism and batching
@pytest.mark.parametrize("surface", [False, True])
def test_plane_align_is_deterministic_batch_chunk_and_cull_independent(surface):
    v, faces = mesh("small_ae.npz")
    n = v.shape[0]
    B = 16
    x = scan_ref.model_points(v, B, seed=3)
    counts = [2125 - 61 * b for b in range(B)]                              # the first bodies span two ranges
    clouds = [AS.moved_surface_scan(x[b, :n], faces, A.SIMILARITY_CASES[b % 3], m=counts[b], seed=7 + b)[0] for b in range(B)]
    xd = torch.from_numpy(x).to(DEV)
    sb = scan.ScanBatch(clouds, DEV)
    ft = scan.FaceTable(faces, n, DEV)
    kw = dict(mode="similarity", iters=6, w_model_to_scan=1.0, trunc=0.5, step="plane")
    kw.update(dict(faces=ft) if surface else dict(normal_faces=ft))
    p1, a1, l1 = scan.align(xd, sb, **kw)
    p2, a2, l2 = scan.align(xd, sb, **kw)
    assert same(p1.packed, p2.packed) and same(p1.scale, p2.scale) and same(l1, l2) and same(a1.points, a2.points) and same(p1.solved, p2.solved)
    assert torch.isfinite(l1).all() and torch.isfinite(p1.packed).all() and (p1.solved == 1).all()
    for b in (0, 5, 15):
        ps, as_, ls = scan.align(xd[b:b + 1], scan.ScanBatch([clouds[b]], DEV), **kw)        # alone, and with M = its own count
        assert same(ps.packed[0], p1.packed[b]) and same(ps.scale[0], p1.scale[b]), b
        assert same(ls[:, 0], l1[:, b]) and same(ps.solved[:, 0], p1.solved[:, b]), b
        assert same(as_.points[0], a1.points[b, :counts[b]]), b
    for chunks in (1, 2, 7):                                                # against the automatic split of the runs above
        pc, _, lc = scan.align(xd[:2], sb.select(slice(0, 2)), chunks=chunks, **kw)
        assert same(pc.packed, p1.packed[:2]) and same(lc, l1[:, :2]) and same(pc.solved, p1.solved[:, :2]), chunks
    if surface:
        pa, aa, la = scan.align(xd[:2], sb.select(slice(0, 2)), cull=True, **kw)
        pb, ab, lb = scan.align(xd[:2], sb.select(slice(0, 2)), cull=False, **kw)
        assert same(pa.packed, pb.packed) and same(pa.scale, pb.scale) and same(la, lb) and same(aa.points, ab.points) and same(pa.solved, pb.solved)


# ------------------------------------------------------------------------------------------------ 5. recovery
@functools.lru_cache(maxsize=None)
def recovery_runs():
    """The GPU plane loop on the four study cases (10 iterations), and on the host the float64 point-to-point loop after 40
    iterations and the float64 plane loop after 10 - each once."""
    x, faces, n, moved, xd, sb, ft = study_batch()
    pose, _, log = scan.align(xd, sb, mode="similarity", iters=10, w_model_to_scan=0.0, faces=ft, step="plane")
    e_point, e_plane = [], []
    for k in range(4):
        xb = x[k, :n].astype(np.float64)
        e_point.append(float(AP.point_errors(xb, faces, moved[k], at=(40,))[0]))
        e_plane.append(float(AP.plane_errors(xb, faces, moved[k], iters=10)[0][-1]))
    return pose, log.cpu().numpy(), e_point, e_plane


@pytest.mark.parametrize("k", range(4))
def test_plane_align_recovers_the_study_cases(k):
    """Measured on the MI355X: see the printed line (and DESIGN 4m)."""
    x, faces, n, moved, xd, sb, ft = study_batch()
    pose, log, e_point, e_plane = recovery_runs()
    s, pts, _, extent = moved[k]
    e_gpu = AS.pose_error(pose.A[k].double().cpu().numpy(), pose.t[k].double().cpu().numpy(), s, pts) / extent
    print("plane recovery %s: pose error %.3g of the extent after 10 iterations; float64 point-to-point after 40: %.3g; float64 plane after 10: "
          "%.3g (GPU / float64 plane %.3g); solved %s; log %.3g -> %.3g"
          % (A.SIMILARITY_CASES[k], e_gpu, e_point[k], e_plane[k], e_gpu / e_plane[k], pose.solved[:, k].cpu().numpy(), log[0, k], log[-1, k]))
    assert (pose.solved[:, k] == 1).all()
    assert e_gpu < e_point[k], (e_gpu, e_point[k])


# ------------------------------------------------------------------------------------------------ 6. vertex form
@pytest.mark.parametrize("w", [0.0, 1.0])
def test_plane_align_in_vertex_form_matches_the_float64_loop(w):
    v, faces = mesh("small_ae.npz")
    n = v.shape[0]
    x = scan_ref.model_points(v, 4, seed=3)
    moved = [A.moved_scan(x[k, :n], case, seed=100 + k) for k, case in enumerate(A.SIMILARITY_CASES)]
    xd = torch.from_numpy(x).to(DEV)
    sb = scan.ScanBatch([mv[0] for mv in moved], DEV)
    pose, _, _ = scan.align(xd, sb, mode="similarity", iters=20, w_model_to_scan=w, normal_faces=faces, step="plane")
    for b, case in enumerate(A.SIMILARITY_CASES):
        xb = x[b, :n].astype(np.float64)
        r_gpu = final_rms(pose, b, moved[b][0], xb)
        Af, tf, _, _ = AP.icp_plane(xb, faces, moved[b][0], "similarity", 20, "moments", w, normals="vertex")
        r_ref = A.rms_scan_to_model(A.apply(Af, tf, moved[b][0].astype(np.float64)), xb)
        print("vertex-form plane %s w=%g: RMS %.5f, float64 plane ICP %.5f (x %.4f)" % (case, w, r_gpu, r_ref, r_gpu / r_ref))
        assert r_gpu <= 1.05 * r_ref, (case, r_gpu, r_ref)                 # test_align.test_align_recovers_the_moved_scans' tolerance


# ------------------------------------------------------------------------------------------------ 7. register_scan
@functools.lru_cache(maxsize=None)
def small_model():
    g = np.load(os.path.join(GOLD, "small_ae.npz"))
    h = load_hierarchy(os.path.join(GOLD, "small_ae.npz"))
    m = sh.SpiralAutoencoder([[3, 16, 32, 64, 128], [[], [], [], [], []]], [[128, 64, 32, 32, 16], [[], [], [], [], 3]], 16, h.sizes, h.spiral_sizes,
                             h.spirals, h.D, h.U, torch.device(DEV))
    m.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w0/")})
    m.set_compute_dtype(torch.float32)
    faces = np.asarray(h.faces, np.int64)
    with torch.no_grad():
        z_star = m.encode(torch.from_numpy(g["x"])[:1].to(DEV).contiguous())
        x_star = m.decode(z_star)
    n = x_star.shape[1] - 1
    pts = S.sample_surface(x_star[0, :n].cpu().numpy(), faces, 2000, seed=5).astype(np.float64)
    At, tt = A.true_pose(MOVES[0], float((pts.max(0) - pts.min(0)).max()))
    cloud = A.apply(*A.inverse(At, tt), pts).astype(np.float32)
    return m, z_star, x_star, n, faces, cloud


def mean_surface_distance(m, z, pose, cloud, n, faces):
    with torch.no_grad():
        xh = m.decode(z)[0, :n].double().cpu().numpy()
    moved = A.apply(pose.A[0].double().cpu().numpy(), pose.t[0].double().cpu().numpy(), cloud.astype(np.float64))
    return float(np.sqrt(S.closest_f64(moved, xh, faces)[1]).mean())


def test_register_scan_with_the_plane_step():
    m, z_star, x_star, n, faces, cloud = small_model()
    z0 = (z_star * 0.9).contiguous()
    sb = scan.ScanBatch([cloud], DEV)
    kw = dict(steps=20, lr=2e-3, faces=faces, align_on="surface", align_iters=5)
    zp, pose_p, fp, lp = editing.register_scan(m, z0, None, sb, align_step="plane", **kw)
    zq, pose_q, fq, lq = editing.register_scan(m, z0, None, sb, align_step="point", **kw)
    zd, pose_d, fd, ld = editing.register_scan(m, z0, None, sb, **kw)
    assert same(zq, zd) and same(pose_q.packed, pose_d.packed) and same(pose_q.scale, pose_d.scale) and same(fq, fd) and same(lq, ld)
    assert torch.isfinite(lp).all() and torch.isfinite(fp).all() and not same(pose_p.packed, pose_q.packed)
    d_plane = mean_surface_distance(m, zp, pose_p, cloud, n, faces)
    d_point = mean_surface_distance(m, zq, pose_q, cloud, n, faces)
    print("register_scan after 5 + 20 steps: mean surface distance plane %.4g, point %.4g; final surface Chamfer %.4g / %.4g"
          % (d_plane, d_point, float(fp[0]), float(fq[0])))
    assert d_plane <= d_point, (d_plane, d_point)
    zv, pose_v, fv, lv = editing.register_scan(m, z0, None, sb, align_step="plane", steps=3, lr=2e-3, normal_faces=faces, align_iters=2,
                                               w_model_to_scan=0.5)                       # vertex pairs, normals from normal_faces
    assert torch.isfinite(lv).all() and torch.isfinite(pose_v.packed).all()


# ------------------------------------------------------------------------------------------------ 8. off means off
def test_off_means_off_and_pose_update_takes_the_step():
    x, faces, n, moved, xd, sb, ft = study_batch()
    for kw in (dict(), dict(faces=ft), dict(faces=ft, w_model_to_scan=0.0)):
        pa, aa, la = scan.align(xd, sb, iters=4, **kw)
        pb, ab, lb = scan.align(xd, sb, iters=4, step="point", **kw)
        assert same(pa.packed, pb.packed) and same(pa.scale, pb.scale) and same(la, lb) and same(aa.points, ab.points)
        assert pa.solved is None and pb.solved is None
    for surface in (False, True):
        poses = []
        for extra in (dict(), dict(step="point"), dict(step="plane")):
            pose = scan.moment_pose(sb, xd, n)
            al = pose.apply(sb)
            matches = {}
            scan.chamfer(xd, al, matches=matches, w_model_to_scan=0.5, **(dict(faces=ft) if surface else dict(normal_faces=ft)))
            assert isinstance(matches["normal_faces"], scan.FaceTable)
            solved = torch.full((4,), -1, dtype=torch.int32, device=DEV)
            scan.pose_update(pose, sb, al, matches, surface=surface, **extra, **(dict(solved=solved) if extra.get("step") == "plane" else {}))
            poses.append((pose, al))
        assert same(poses[0][0].packed, poses[1][0].packed) and same(poses[0][0].scale, poses[1][0].scale)
        assert same(poses[0][1].points, poses[1][1].points)
        assert not same(poses[0][0].packed, poses[2][0].packed) and (solved == 1).all()
        assert same(poses[2][1].points, poses[2][0].apply(sb).points)     # the aligned scan is the original under the new pose


def test_argument_errors():
    x, faces, n, moved, xd, sb, ft = study_batch()
    with pytest.raises(ValueError, match="normal_faces"):
        scan.align(xd, sb, step="plane")                                    # vertex form without a face table
    with pytest.raises(ValueError, match="step"):
        scan.align(xd, sb, step="planar")
    normals = [np.tile(np.array([[0.0, 0.0, 1.0]]), (len(mv[0]), 1)) for mv in moved]
    with pytest.raises(ValueError, match="not built"):
        scan.align(xd, scan.ScanBatch([mv[0] for mv in moved], DEV, normals=normals), faces=faces, normal_angle=60.0, normal_faces=faces,
                   trunc=0.1, step="plane")
    matches = {}
    scan.chamfer(xd, sb, matches=matches)                                  # no face table anywhere: no normals to be had
    with pytest.raises(ValueError, match="normals"):
        scan.pose_update(scan.Pose.identity(4, DEV), sb, scan.Pose.identity(4, DEV).apply(sb), matches, step="plane")
