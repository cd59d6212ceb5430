"""Scan alignment on the GPU: the moments and the closed-form pose against float64, the transform against its host mirror,
descent and recovery of scan.align, determinism and batching, editing.register_scan against fit_scan on unmoved scans, the
kernels a step launches, and one run at the size tools/bench_align.py times."""
import os

import numpy as np
import pytest
import torch

import semantichuman_amd as sh
from semantichuman_amd import _lib
from semantichuman_amd import constants as C
from semantichuman_amd import editing, ops, scan, synthetic
from semantichuman_amd.hierarchy import load_hierarchy
from tests import align_ref as A
from tests import scan_ref as R
from tests.launch_record import launch_counts as launches

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
SCALED = [2, 3, 4]
PARTS = list(range(1, 16))
U24, U53 = 2.0 ** -24, 2.0 ** -53
MODES = ["translation", "rigid", "similarity"]


def ragged_counts(B, M):
    return [max(1, (M * (B - b)) // B - (b % 3)) if b else M for b in range(B)]


def verts_of(name):
    return np.asarray(load_hierarchy(os.path.join(GOLD, name)).verts, dtype=np.float64)


def searches(sb, xd, n, vmask, w):
    i_sm, d_sm = ops.nearest_points(sb.points, xd, q_count=sb.counts, t_mask=vmask, nt=n)
    i_ms, d_ms = ops.nearest_points(xd, sb.points, t_count=sb.counts) if w > 0 else (None, None)
    return i_sm, d_sm, i_ms, d_ms


def gpu_moments(sb, xd, n, vmask, m, tau2, w, mode="similarity", pose=None):
    """(mom [B, 20] float64, inc [B, 13], pose_out [B, 12], scale_out [B]) from given matches m = (i_sm, d_sm, i_ms, d_ms)."""
    B = xd.shape[0]
    vm, vsb = ops._mask_arg(vmask, B, n, xd.device)
    part = ops.align_moments(sb.points, sb.counts, xd, n, vm, vsb, m[0], m[1], m[2], m[3], tau2, w)
    assert not torch.isnan(part).any()
    mom = torch.full((B, 20), float("nan"), dtype=torch.float64, device=DEV)
    inc = torch.full((B, 13), float("nan"), device=DEV)
    pose = scan.Pose.identity(B, DEV) if pose is None else pose
    out, sc = torch.full((B, 12), float("nan"), device=DEV), torch.full((B,), float("nan"), device=DEV)
    ops.align_solve(part, sb.points.shape[1], n, sb.counts, w, mode, pose.packed, pose.scale, out, sc, inc, mom)
    return mom.cpu().numpy(), inc.cpu().numpy().astype(np.float64), out.cpu().numpy(), sc.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. moments against float64
@pytest.mark.parametrize("M", [1, 63, 1000, 20011])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_moments_against_float64(B, M):
    v = verts_of("template6890.npz")
    n = v.shape[0]
    x = R.model_points(v, B, seed=3)
    counts = ragged_counts(B, M)
    clouds = R.make_scans(x, n, counts, seed=100 + M)
    sb = scan.ScanBatch(clouds, DEV)
    xd = torch.from_numpy(x).to(DEV)
    rs = np.random.RandomState(7)
    worst = 0.0
    for masked in (False, True):
        vmask = rs.rand(n) < 0.7 if masked else None
        for w in (0.0, 0.5):
            m = searches(sb, xd, n, vmask, w)
            mh = [None if t is None else t.cpu().numpy() for t in m]
            for truncate in (False, True):
                tau2 = float(np.float32(np.median(mh[1][0, :counts[0]]))) if truncate else float("inf")
                mom, _, _, _ = gpu_moments(sb, xd, n, vmask, m, tau2, w)
                for b in range(B):
                    p, q, wt = A.pairs(clouds[b], x[b], n, counts[b], vmask, mh[0][b], mh[1][b], None if mh[2] is None else mh[2][b],
                                       None if mh[3] is None else mh[3][b], tau2, w)
                    ref, mag = A.moments(p, q, wt)
                    K = len(wt)
                    assert mom[b, 18] == K and mom[b, 19] == 0.0, (b, mom[b, 18], K)               # the kept count is exact
                    # Derived: every product of two fp32 values is exact in fp64, so kernel and host differ by the order of a
                    # K-term fp64 sum only: at most (K - 1) 2^-53 sum|term| for either order, plus a few roundings of the weight
                    # and of the three-term |p|^2.  Bound: 2 (K + 16) 2^-53 sum w|term|.
                    bound = 2 * (K + 16) * U53 * mag[:18]
                    err = np.abs(mom[b, :18] - ref[:18])
                    worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                    assert (err <= bound).all(), (b, masked, w, truncate, err, bound)
    print("moments B=%d M=%d: largest error / bound %.3g" % (B, M, worst))


# ------------------------------------------------------------------------------------------------ 2. solve against float64
def check_rotation(inc):
    c = inc[12]
    Rg = inc[:9].reshape(3, 3) / c
    assert np.isfinite(inc).all() and c > 0
    # inc holds fp32 roundings of c R: each entry is off by at most 2^-24 |c R|, a product of two rows by a few times that
    assert np.abs(Rg.T @ Rg - np.eye(3)).max() <= 8 * U24, Rg
    assert abs(np.linalg.det(Rg) - 1.0) <= 8 * U24, np.linalg.det(Rg)
    return Rg, c


@pytest.mark.parametrize("mode", MODES)
def test_solve_against_umeyama(mode):
    v = verts_of("template6890.npz")
    n = v.shape[0]
    B = 4
    x = R.model_points(v, B, seed=3)
    moved = [A.moved_scan(x[b, :n], case, m=3000 + 7 * b, seed=40 + b) for b, case in enumerate(A.SIMILARITY_CASES)]
    clouds = [m[0] for m in moved]
    sb = scan.ScanBatch(clouds, DEV)
    xd = torch.from_numpy(x).to(DEV)
    rs = np.random.RandomState(3)
    start = scan.Pose(torch.from_numpy(np.stack([1.1 * A.rotation(rs.randn(3), 20.0) for _ in range(B)])), torch.from_numpy(rs.randn(B, 3) * 0.1)).select(slice(0, B))
    start = scan.Pose.from_packed(start.packed.to(DEV), start.scale.to(DEV))
    w = 0.5
    m = searches(sb, xd, n, None, w)
    mom, inc, out, sc = gpu_moments(sb, xd, n, None, m, float("inf"), w, mode, start)
    for b in range(B):
        Rg, c = check_rotation(inc[b])
        Ar, tr, cr, Rr = A.umeyama(mom[b], mode)
        p = clouds[b].astype(np.float64)
        got, ref = A.apply(inc[b, :9].reshape(3, 3), inc[b, 9:12], p), A.apply(Ar, tr, p)
        extent = max(np.abs(ref).max(), np.abs(p).max())
        # the increment is the float64 solution rounded to fp32 entry by entry: a transformed coordinate is three products and
        # a translation, each off by at most 2^-24 of its size -> 4 x 2^-24 x extent; Jacobi against SVD adds ~1e-15.  Bound: 8 x.
        print("solve %s b=%d: |dp| %.3g (bound %.3g), c %.6f vs %.6f" % (mode, b, np.abs(got - ref).max(), 8 * U24 * extent, c, cr))
        assert np.abs(got - ref).max() <= 8 * U24 * extent
        if mode != "similarity":
            assert inc[b, 12] == 1.0
        if mode == "translation":
            assert np.array_equal(inc[b, :9].reshape(3, 3), np.eye(3))
        # composition, rounded once: against float64 composition of the same fp32 inputs
        A0, t0 = start.A[b].double().cpu().numpy(), start.t[b].double().cpu().numpy()
        An, tn = A.compose(Ar, tr, A0, t0)
        assert np.abs(out[b, :9].reshape(3, 3) - An).max() <= 4 * U24 * np.abs(An).max()
        assert np.abs(out[b, 9:] - tn).max() <= 4 * U24 * max(np.abs(tn).max(), np.abs(tr).max(), 1.0)
        assert abs(sc[b] - cr * float(start.scale[b])) <= 4 * U24 * sc[b]


def hand_pairs(ps, qs):
    """Bodies whose pairs are given by hand: scan point j matched to model row j, all distances zero (kept)."""
    B, K = len(ps), max(len(p) for p in ps)
    s = np.zeros((B, K, 3), np.float32)
    x = np.zeros((B, K + 1, 3), np.float32)
    for b in range(B):
        s[b, :len(ps[b])] = ps[b]; x[b, :len(qs[b])] = qs[b]
    cnt = [len(p) for p in ps]
    sb = scan.ScanBatch([s[b, :max(c, 1)] for b, c in enumerate(cnt)], DEV)
    sb.counts = torch.tensor(cnt, dtype=torch.int32, device=DEV)
    idx = torch.arange(sb.points.shape[1], dtype=torch.int32, device=DEV).expand(B, -1).contiguous()
    d2 = torch.zeros((B, sb.points.shape[1]), device=DEV)
    return sb, torch.from_numpy(x).to(DEV), K, (idx, d2, None, None), s, x, cnt


@pytest.mark.parametrize("mode", MODES)
def test_solve_degenerate_inputs(mode):
    rs = np.random.RandomState(5)
    line = np.outer(np.linspace(-1, 1, 5), [0.3, -0.2, 0.9])
    plane = np.concatenate([rs.randn(6, 2), np.zeros((6, 1))], 1)
    cloud = rs.randn(40, 3)
    Rt = A.rotation([0.2, -1.0, 0.4], 35.0)
    ps = [cloud[:1], cloud[:2], line, plane, cloud, cloud[:0].reshape(0, 3), cloud[:3] * 0 + cloud[0]]
    qs = [cloud[1:2], A.apply(1.2 * Rt, [0.1, 0.2, 0.3], cloud[:2]), A.apply(Rt, [0.5, 0, 0], line), plane * np.array([1.0, -1.0, 1.0]),
          cloud * np.array([-1.0, 1.0, 1.0]), cloud[:0].reshape(0, 3), cloud[3:6]]
    names = ["one pair", "two pairs", "collinear", "coplanar mirror", "reflected cloud", "no pair", "coincident scan points"]
    sb, xd, K, m, s, x, cnt = hand_pairs(ps, qs)
    start = scan.Pose(torch.from_numpy(np.stack([0.9 * A.rotation(rs.randn(3), 10.0) for _ in ps])), torch.from_numpy(rs.randn(len(ps), 3)))
    start = scan.Pose.from_packed(start.packed.to(DEV), start.scale.to(DEV))
    mom, inc, out, sc = gpu_moments(sb, xd, K, None, m, float("inf"), 0.0, mode, start)
    for b, name in enumerate(names):
        if cnt[b] == 0:                                                    # W == 0: the identity, bitwise, and the pose passes through
            assert mom[b, 0] == 0 and np.array_equal(inc[b], np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1.0])), inc[b]
            assert np.array_equal(out[b], start.packed[b].cpu().numpy()) and sc[b] == float(start.scale[b])
            continue
        check_rotation(inc[b])                                             # a rotation, never a reflection
        p, q = s[b, :cnt[b]].astype(np.float64), x[b, :cnt[b]].astype(np.float64)
        wt = np.full(cnt[b], 1.0 / cnt[b])
        Ar, tr, _, _ = A.umeyama(A.moments(p, q, wt)[0], mode)
        r_gpu = A.residual(p, q, wt, inc[b, :9].reshape(3, 3), inc[b, 9:12])
        r_ref = A.residual(p, q, wt, Ar, tr)
        # the answer need not be unique; the residual is.  The stored increment is rounded to fp32, which moves every
        # transformed point by up to 8 x 2^-24 x extent (see above): that much residual is rounding, the rest must match numpy's.
        extent = max(np.abs(p).max(), np.abs(q).max(), 1.0)
        floor = (8 * U24 * extent) ** 2 + 2 * 8 * U24 * extent * np.sqrt(r_ref)
        print("degenerate %s / %s: residual %.6g, numpy %.6g" % (mode, name, r_gpu, r_ref))
        assert r_gpu <= r_ref * (1 + 1e-6) + floor, (name, r_gpu, r_ref)


# ------------------------------------------------------------------------------------------------ 3. transform
def test_transform_points_bitwise_and_padding():
    rs = np.random.RandomState(11)
    B, M = 5, 1300
    counts = [1300, 0, 1, 257, 1299]
    src = torch.from_numpy(rs.randn(B, M + 3, 3).astype(np.float32)).to(DEV)[:, :M]       # batch stride longer than a body
    pose = np.stack([A.pack(rs.uniform(0.5, 2) * A.rotation(rs.randn(3), rs.uniform(-180, 180)), rs.randn(3)) for _ in range(B)])
    P = scan.Pose.from_packed(torch.from_numpy(pose).to(DEV), torch.ones(B, device=DEV))
    out = torch.full((B, M, 3), float("nan"), device=DEV)
    ops.transform_points(src, torch.tensor(counts, dtype=torch.int32, device=DEV), P.packed, out=out)
    got, sh_ = out.cpu().numpy(), src.cpu().numpy()
    for b in range(B):
        ref = A.transform_f32(pose[b], sh_[b, :counts[b]])
        assert np.array_equal(got[b, :counts[b]].view(np.int32), ref.view(np.int32)), b
        assert (got[b, counts[b]:].view(np.int32) == 0).all(), b                             # +0.0, every row stored
    full = P.apply(src)                                                                      # no counts: every row is live
    assert np.array_equal(full[3].cpu().numpy().view(np.int32), A.transform_f32(pose[3], sh_[3]).view(np.int32))


# ------------------------------------------------------------------------------------------------ shared moved scans
def moved_batch(template, cases, m=20011, half=False, seed0=100):
    v = verts_of(template)
    n = v.shape[0]
    x = R.model_points(v, 4, seed=3)
    moved = [A.moved_scan(x[k, :n], case, m=m, seed=seed0 + k, half=half) for k, case in enumerate(cases)]
    xd = torch.from_numpy(x[:len(cases)]).to(DEV)
    return x, n, moved, xd, scan.ScanBatch([mv[0] for mv in moved], DEV)


# ------------------------------------------------------------------------------------------------ 4. descent
@pytest.mark.parametrize("truncate", [False, True])
@pytest.mark.parametrize("w", [0.0, 1.0])
@pytest.mark.parametrize("mode", MODES)
def test_align_never_raises_the_chamfer_value(mode, w, truncate):
    x, n, moved, xd, sb = moved_batch("template6890.npz", A.SIMILARITY_CASES[:3], m=5000)
    trunc = 0.05 if truncate else None
    pose, aligned, log = scan.align(xd, sb, mode=mode, iters=15, w_model_to_scan=w, trunc=trunc)
    L = log.cpu().numpy().astype(np.float64)
    assert L.shape == (15, 3) and np.isfinite(L).all()
    # Fixed matches, then least squares over the pose, then re-matching: no term of the (truncated) loss can rise - in exact
    # arithmetic.  The transformed points are stored in fp32 (each coordinate off by up to d = 4 x 2^-24 x extent: three products
    # and the translation), which changes a squared distance by up to 2 d sqrt(d2) and so the mean by up to 2 d sqrt(L) (Cauchy-
    # Schwarz), on either side of the comparison; the fp32 rounding of the logged value itself is 2^-24 L.
    extent = float(np.abs(x).max()) * 1.5
    tol = 2 * (2 * 4 * U24 * extent * np.sqrt((1 + w) * L[:-1])) + 2 * U24 * L[:-1]
    rise = L[1:] - L[:-1]
    print("descent %s w=%g trunc=%s: %s -> %s, largest rise / tolerance %.3g" % (mode, w, trunc, L[0], L[-1], float((rise / tol).max())))
    assert (rise <= tol).all(), (rise / tol).max()
    assert (L[-1] < L[0]).all()


# ------------------------------------------------------------------------------------------------ 5. recovery
def final_rms(pose, b, scan_f32, xb):
    Ap, tp = pose.A[b].double().cpu().numpy(), pose.t[b].double().cpu().numpy()
    return A.rms_scan_to_model(A.apply(Ap, tp, scan_f32.astype(np.float64)), xb)


@pytest.mark.parametrize("w", [0.0, 1.0])
@pytest.mark.parametrize("template", ["template6890.npz", "small_ae.npz"])
def test_align_recovers_the_moved_scans(template, w):
    x, n, moved, xd, sb = moved_batch(template, A.SIMILARITY_CASES)
    pose, aligned, log = scan.align(xd, sb, mode="similarity", iters=40, w_model_to_scan=w)
    for b, case in enumerate(A.SIMILARITY_CASES):
        xb = x[b, :n].astype(np.float64)
        r_true = A.rms_scan_to_model(moved[b][1], xb)
        r_gpu = final_rms(pose, b, moved[b][0], xb)
        Af, tf = A.icp(xb, moved[b][0], "similarity", 40, "moments", w)
        r_ref = A.rms_scan_to_model(A.apply(Af, tf, moved[b][0].astype(np.float64)), xb)
        print("recovery %s %s w=%g: RMS %.5f, at the true pose %.5f (x %.4f), float64 ICP %.5f (x %.4f)"
              % (template, case, w, r_gpu, r_true, r_gpu / r_true, r_ref, r_gpu / r_ref))
        assert r_gpu <= 1.05 * r_true, (case, r_gpu, r_true)
        assert r_gpu <= 1.05 * r_ref, (case, r_gpu, r_ref)
        assert abs(float(pose.scale[b]) - np.cbrt(np.linalg.det(pose.A[b].double().cpu().numpy()))) <= 1e-4 * float(pose.scale[b])


def test_align_rigid_on_half_scans():
    cases = [(d, 1.0, f) for d, f in A.RIGID_HALF_CASES]
    x, n, moved, xd, sb = moved_batch("template6890.npz", cases, half=True)
    pose, aligned, log = scan.align(xd, sb, mode="rigid", iters=40, init="identity", w_model_to_scan=0.0)
    for b, case in enumerate(cases):
        xb = x[b, :n].astype(np.float64)
        r_true = A.rms_scan_to_model(moved[b][1], xb)
        r_start = A.rms_scan_to_model(moved[b][0].astype(np.float64), xb)
        r_gpu = final_rms(pose, b, moved[b][0], xb)
        Af, tf = A.icp(xb, moved[b][0], "rigid", 40, "identity", 0.0)
        r_ref = A.rms_scan_to_model(A.apply(Af, tf, moved[b][0].astype(np.float64)), xb)
        print("half scan %s: RMS %.5f -> %.5f, at the true pose %.5f, float64 ICP %.5f" % (case, r_start, r_gpu, r_true, r_ref))
        assert r_gpu <= 1.05 * r_true and r_gpu <= 1.05 * r_ref and r_gpu < r_start
        assert float(pose.scale[b]) == 1.0


# ------------------------------------------------------------------------------------------------ 6. determinism and batching
def test_align_is_deterministic_batch_independent_and_chunk_independent():
    v = verts_of("template6890.npz")
    n = v.shape[0]
    B = 16
    x = R.model_points(v, B, seed=3)
    counts = ragged_counts(B, 20011)
    clouds = [A.moved_scan(x[b, :n], A.SIMILARITY_CASES[b % 3], m=counts[b], seed=7 + b)[0] for b in range(B)]
    xd = torch.from_numpy(x).to(DEV)
    sb = scan.ScanBatch(clouds, DEV)
    kw = dict(mode="similarity", iters=8, w_model_to_scan=1.0, trunc=0.2)
    p1, a1, l1 = scan.align(xd, sb, **kw)
    p2, a2, l2 = scan.align(xd, sb, **kw)
    assert torch.equal(p1.packed, p2.packed) and torch.equal(p1.scale, p2.scale) and torch.equal(l1, l2) and torch.equal(a1.points, a2.points)
    for b in (0, 5, 11, 15):
        ps, as_, ls = scan.align(xd[b:b + 1], scan.ScanBatch([clouds[b]], DEV), **kw)       # alone, and with M = its own count
        assert torch.equal(ps.packed[0], p1.packed[b]) and torch.equal(ps.scale[0], p1.scale[b]), b
        assert torch.equal(ls[:, 0], l1[:, b]), b
        assert torch.equal(as_.points[0], a1.points[b, :counts[b]]), b
    for chunks in (1, 3, 7):
        pc, _, lc = scan.align(xd[:2], sb.select(slice(0, 2)), chunks=chunks, **kw)
        assert torch.equal(pc.packed, p1.packed[:2]) and torch.equal(lc, l1[:, :2]), chunks


# ------------------------------------------------------------------------------------------------ 7. register_scan
def semantic_setup(B=3, seed=0):
    """tests/test_scan.py's recipe: the semantic.npz model, z* = encode(x), scans = the decoded vertices in a random order, the
    start = z* with parts 2, 3, 4 scaled by 1.3."""
    dev = torch.device(DEV)
    gs = np.load(os.path.join(GOLD, "semantic.npz"))
    h = load_hierarchy(os.path.join(GOLD, "semantic.npz"))
    coarse = {n: gs["part_coarse_%d" % k] for k, n in enumerate(C.PART_LIST)}
    m = sh.SpiralAutoencoder_multiz_partkps(C.KPS_INDEX_LIST, coarse, C.FILTER_SIZES_ENC, C.FILTER_SIZES_DEC, 8, 8, h.sizes,
                                            h.spiral_sizes, h.spirals, h.D, h.U, dev)
    m.load_state_dict({k[3:]: torch.from_numpy(gs[k]) for k in gs.files if k.startswith("w0/")})
    m.set_compute_dtype(torch.float32)
    idx = torch.arange(B) % 3
    gen = torch.Generator().manual_seed(seed)
    x = torch.from_numpy(gs["x"])[idx]
    if B > 3:
        x = x * (1 + 0.05 * torch.randn((B, 1, 3), generator=gen))
    x = x.to(dev).contiguous()
    kps = torch.from_numpy(gs["kps"])[idx].to(dev).contiguous()
    with torch.no_grad():
        z_star, z_kps, dummy = m.encode(x, kps)
        x_star = m.decode(z_star, z_kps, dummy)
    n = x_star.shape[1] - 1
    perm = [torch.randperm(n, generator=gen) for _ in range(B)]
    clouds = [x_star[b, :n].cpu().numpy()[perm[b].numpy()] for b in range(B)]
    z0 = editing.edit_part_size(z_star, SCALED, 1.3)
    return m, z0, z_kps, dummy, clouds, x_star, n


MOVES = [(10.0, 1.1, 0.1), (20.0, 1.2, 0.3), (15.0, 0.9, 0.2)]


def move_clouds(clouds):
    """Every cloud carried into a frame of its own by the inverse of a known similarity (MOVES, cycled)."""
    out = []
    for b, c in enumerate(clouds):
        c64 = c.astype(np.float64)
        At, tt = A.true_pose(MOVES[b % 3], (c64.max(0) - c64.min(0)).max())
        out.append(A.apply(*A.inverse(At, tt), c64).astype(np.float32))
    return out


def snapshot(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


def vertex_distance(m, z, z_kps, dummy, x_star, n):
    with torch.no_grad():
        return (m.decode(z, z_kps, dummy)[:, :n] - x_star[:, :n]).norm(dim=2).mean().item()


def test_register_scan_recovers_the_body_like_fit_scan_on_unmoved_scans():
    """Measured on the MI355X: see the printed line (and DESIGN 4i)."""
    m, z0, z_kps, dummy, clouds, x_star, n = semantic_setup()
    unmoved, moved = scan.ScanBatch(clouds, DEV), scan.ScanBatch(move_clouds(clouds), DEV)
    before = snapshot(m)
    name0 = next(iter(before))
    sentinel = torch.full_like(before[name0], 7.0)
    dict(m.named_parameters())[name0].grad = sentinel
    list(m.parameters())[1].requires_grad_(False)
    flags = {k: p.requires_grad for k, p in m.named_parameters()}
    z_in, zk_in = z0.clone(), z_kps.clone()
    zu, _, _ = editing.fit_scan(m, z0, z_kps, unmoved, parts=PARTS, steps=800, lr=2e-3, dummy=dummy)              # the yardstick
    zr, pose, final, losses = editing.register_scan(m, z0, z_kps, moved, parts=PARTS, steps=800, lr=2e-3, dummy=dummy)
    zm, _, _ = editing.fit_scan(m, z0, z_kps, moved, parts=PARTS, steps=100, lr=2e-3, dummy=dummy)                # no alignment
    assert losses.is_cuda and losses.shape == (800,) and tuple(final.shape) == (3,) and len(pose) == 3
    l = losses.cpu()
    assert torch.isfinite(l).all() and torch.isfinite(final).all() and float(l[-1]) < float(l[0])
    d_u, d_r, d_m, d_0 = (vertex_distance(m, z, z_kps, dummy, x_star, n) for z in (zu, zr, zm, z0))
    # (a) The floor: the scan reaches the loss through fp32 roundings that fit_scan on unmoved scans never sees - the moved
    # points stored in fp32 (2^-24 of their size), the 12 stored pose entries (a transformed coordinate is three products and a
    # translation: 4 x 2^-24 x extent) and the three fused steps of the transform (3 x 2^-24 x extent): 8 x 2^-24 x extent.
    extent = float(x_star[:, :n].abs().max()) * 1.3
    floor = 8 * U24 * extent
    print("register_scan: loss %.4g -> %.4g; mean vertex distance to x*: start %.4g, fit_scan on unmoved scans %.4g, register_scan on "
          "moved scans %.4g (bound max(1.10 x, floor %.3g)), fit_scan on moved scans %.4g" % (float(l[0]), float(l[-1]), d_0, d_u, d_r, floor, d_m))
    assert d_r <= max(1.10 * d_u, floor), (d_r, d_u, floor)
    assert d_m > 100 * max(d_r, floor) and d_m > d_0, (d_m, d_r, d_0)                                           # (b) the misalignment matters
    # (d) nothing else moved
    others = [k for k in range(z0.shape[1]) if k not in PARTS]
    assert torch.equal(zr[:, others], z0[:, others]) and not torch.equal(zr[:, PARTS], z0[:, PARTS])
    assert torch.equal(z0, z_in) and torch.equal(z_kps, zk_in)
    for k, p in m.named_parameters():
        assert torch.equal(p.detach(), before[k]), k
        assert p.requires_grad == flags[k], k
    assert dict(m.named_parameters())[name0].grad is sentinel and torch.all(sentinel == 7.0)
    assert all(p.grad is None for k, p in m.named_parameters() if k != name0)


def test_register_scan_result_lies_on_the_moved_scan():
    """(c) after a short fit (the Chamfer value is still far above rounding): the value in the scan's frame x scale^2 is the
    model-frame value."""
    m, z0, z_kps, dummy, clouds, x_star, n = semantic_setup()
    moved = scan.ScanBatch(move_clouds(clouds), DEV)
    zr, pose, final, _ = editing.register_scan(m, z0, z_kps, moved, parts=PARTS, steps=40, lr=2e-3, dummy=dummy, w_model_to_scan=0.5)
    with torch.no_grad():
        x_hat = m.decode(zr, z_kps, dummy)
        again = scan.chamfer(x_hat, pose.apply(moved), w_model_to_scan=0.5)
        back = pose.to_scan_frame(x_hat).contiguous()
        in_scan = scan.chamfer(back, moved, w_model_to_scan=0.5) * pose.scale ** 2
    assert torch.equal(again, final)
    f, g = final.double().cpu().numpy(), in_scan.double().cpu().numpy()
    # both sides see points rounded to fp32 after a transform (d = 8 x 2^-24 x extent as above, here on scan AND model points):
    # a mean of squared distances L moves by up to 2 (2 d) sqrt(L) (1 + w)
    extent = float(x_star.abs().max()) * 1.3
    tol = 2 * (2 * 8 * U24 * extent) * np.sqrt(1.5 * f) * 1.5
    print("scan frame x scale^2 %s, model frame %s, |diff| / tolerance %s" % (g, f, np.abs(g - f) / tol))
    assert (f > 1e-8).all() and (np.abs(g - f) <= tol).all()


def test_batched_register_scan_matches_single_body_runs():
    B = 16
    m, z0, z_kps, dummy, clouds, x_star, n = semantic_setup(B=B, seed=4)
    moved = move_clouds(clouds)
    sb = scan.ScanBatch(moved, DEV)
    zb, pb, fb, _ = editing.register_scan(m, z0, z_kps, sb, parts=PARTS, steps=60, lr=1e-2, dummy=dummy)
    for b in (0, 5, 11):
        s = slice(b, b + 1)
        z1, p1, f1, _ = editing.register_scan(m, z0[s], z_kps[s], sb.select(s), parts=PARTS, steps=60, lr=1e-2, dummy=dummy[s])
        print("batched vs single b=%d: |dz| %.3g of %.3g, chamfer %.6g vs %.6g, |dpose| %.3g" % (
            b, float((z1 - zb[s]).abs().max()), float(zb[s].abs().max()), float(f1), float(fb[b]), float((p1.packed - pb.packed[s]).abs().max())))
        assert float((z1 - zb[s]).abs().max()) <= 1e-5 * float(zb[s].abs().max()), b
        assert float(((f1 - fb[s]) / fb[s]).abs().max()) <= 1e-5, b


# ------------------------------------------------------------------------------------------------ 8. what ran
def test_register_scan_step_runs_the_new_kernels_no_extra_search_and_leaves_fit_scan_alone():
    m, z0, z_kps, dummy, clouds, _, _ = semantic_setup()
    unmoved, moved = scan.ScanBatch(clouds, DEV), scan.ScanBatch(move_clouds(clouds), DEV)
    kw = dict(parts=PARTS, steps=5, lr=1e-2, w_model_to_scan=0.5, dummy=dummy)

    a, n_fit = launches(lambda: editing.fit_scan(m, z0, z_kps, unmoved, **kw))
    r, n_reg = launches(lambda: editing.register_scan(m, z0, z_kps, moved, align_iters=0, align_every=1, **kw))
    b = editing.fit_scan(m, z0, z_kps, unmoved, **kw)
    for u, w in zip(a, b):
        assert torch.equal(u, w)                                           # fit_scan before and after a register_scan call: same bits
    print("fit_scan launches %s\nregister_scan launches %s" % (sorted(n_fit.items()), sorted(n_reg.items())))
    # 5 steps and the final evaluation search twice each in both functions; the 5 pose updates add no search
    assert n_reg["nearest_search_kernel"] == n_fit["nearest_search_kernel"] == 12
    assert n_reg["align_moments_kernel"] == 5 and n_reg["align_solve_kernel"] == 5
    assert n_reg["transform_points_kernel"] == 5 + 1                       # + the start pose applied once
    assert not [k for k in n_fit if k.startswith(("align_", "transform_points"))]
    assert not [k for k in n_reg if k.startswith("wgrad") or "bwd_wgt" in k or "slab_reduce" in k], sorted(n_reg)
    r2 = editing.register_scan(m, z0, z_kps, moved, align_iters=0, align_every=1, **kw)
    assert torch.equal(r[0], r2[0]) and torch.equal(r[1].packed, r2[1].packed) and torch.equal(r[3], r2[3])
    # align_every = 0 keeps the start pose bitwise
    start = scan.moment_pose(moved, editing._decode(m, z0, z_kps, dummy).detach())
    r3 = editing.register_scan(m, z0, z_kps, moved, align_iters=0, align_every=0, init=start, **kw)
    assert torch.equal(r3[1].packed, start.packed) and torch.equal(r3[1].scale, start.scale)


# ------------------------------------------------------------------------------------------------ 9. at size
@pytest.mark.parametrize("f32_mma", ["planes3"], indirect=True)
def test_register_scan_at_size(f32_mma):
    """20 steps with a pose update after each on the 6890-vertex plain autoencoder, 16 bodies against 50 000-point scans moved by a
    similarity: the shape tools/bench_align.py times."""
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
    gen = torch.Generator().manual_seed(1)
    pick = torch.randint(0, n, (B, M), generator=gen).to(dev)
    pts = torch.gather(x_star[:, :n], 1, pick[:, :, None].expand(-1, -1, 3))
    At, tt = A.true_pose((10.0, 1.1, 0.1), float(pts.amax() - pts.amin()))
    Ai, ti = A.inverse(At, tt)
    true = scan.Pose(torch.from_numpy(Ai)[None].expand(B, -1, -1).contiguous(), torch.from_numpy(ti)[None].expand(B, -1).contiguous())
    scans = scan.ScanBatch(scan.Pose.from_packed(true.packed.to(dev), true.scale.to(dev)).apply(pts), dev)
    before = snapshot(m)
    z0 = z_star * 1.3
    z1, pose, final, losses = editing.register_scan(m, z0, None, scans, steps=20, lr=1e-2, w_model_to_scan=0.5, align_iters=10, align_every=1)
    l = losses.cpu()
    print("register_scan at size: loss %.5g -> %.5g, scale %s" % (float(l[0]), float(l[-1]), pose.scale[:3].cpu().numpy()))
    assert torch.isfinite(l).all() and torch.isfinite(final).all() and float(l[-1]) < float(l[0]), (float(l[0]), float(l[-1]))
    assert torch.isfinite(pose.packed).all() and z1.shape == z0.shape and not torch.equal(z1, z0)
    for k, p in m.named_parameters():
        assert torch.equal(p.detach(), before[k]) and p.requires_grad and p.grad is None, k
