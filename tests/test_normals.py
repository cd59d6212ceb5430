"""Matching by normal on the GPU: sh_vertex_normals against float64, sh_nearest_points_gated against the host reference
(bitwise), the open gate, split and batching invariance, a query with no compatible target, the thin slab the ungated search
gets wrong, off-means-off, 180 degrees = no gate, normals under a pose, and the argument errors."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, editing, ops, scan
from semantichuman_amd.hierarchy import load_hierarchy
from tests import normals_ref as N
from tests import scan_ref
from tests.launch_record import recorded
from tests.test_scan import PARTS, semantic_setup

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
NEW_KERNELS = {"nearest_search_gated_kernel", "vertex_normals_kernel"}


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return all(torch.equal(bits(u), bits(v)) for u, v in zip(a, b))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ G1
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", N.TEMPLATES)
def test_vertex_normals_against_float64(name, B):
    x, f = N.bodies(name, B)
    n = x.shape[1] - 1
    x[:, n] = np.nan                                                       # the dummy row: a kernel that addressed it would show
    nrm = scan.vertex_normals(dev(x), f).cpu().numpy()
    assert nrm.shape == (B, n, 3) and np.isfinite(nrm).all()
    worst = max(float(N.angle(nrm[b], N.normals_f64(x[b, :n], f)).max()) for b in range(B))
    bound = N.KERNEL_FACTOR * N.F32_ANGLE
    print("vertex_normals %s B=%d: largest angle to float64 %.3e rad = %.1f %% of the bound %.3e"
          % (name, B, worst, 100 * worst / bound, bound))
    assert worst <= bound
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=2) - 1).max() <= 2.0 ** -22


def test_vertex_normals_edge_cases_and_batching():
    # vertices 0..3: a square in z = 0 (normal exactly +z); 4: in no face; 5..8: a fan of zero-area (collinear) faces; row 9: dummy
    x = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [5, 5, 5], [0, 0, 1], [1, 1, 2], [2, 2, 3], [3, 3, 4], [7, 7, 7]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [5, 6, 7], [5, 7, 8]])
    xd = dev(x[None])
    xd[0, 9] = float("nan")
    nrm = scan.vertex_normals(xd, f).cpu().numpy()[0]
    assert nrm.shape == (9, 3)
    assert np.array_equal(nrm[:4], np.tile(np.float32([0, 0, 1]), (4, 1)))
    assert (nrm[4:] == 0).all() and not np.signbit(nrm[4:]).any()
    assert np.array_equal(nrm, N.normals_f32(x[:9], f))
    # n given explicitly for a bare vertex tensor, and a FaceTable reused
    ft = scan.FaceTable(f, 9, DEV)
    assert torch.equal(scan.vertex_normals(dev(x[None, :9]), ft), dev(nrm[None]))
    # a body alone and as one of 16: the same bits
    xb, fb = N.bodies("small_ae.npz", 16)
    all16 = scan.vertex_normals(dev(xb), fb)
    for b in (0, 7, 15):
        assert same([scan.vertex_normals(dev(xb[b:b + 1]), fb)], [all16[b:b + 1]])


# ------------------------------------------------------------------------------------------------ G2, G3
@functools.lru_cache(maxsize=None)
def search_case(nq, nt, B, masked):
    """Points, unit normals with some zero rows, ragged counts on both sides, a per-body target mask."""
    rs = np.random.RandomState(1000 * nq + 10 * nt + B + (5 if masked else 0))
    q = rs.randn(B, nq, 3).astype(np.float32)
    t = rs.randn(B, nt, 3).astype(np.float32)
    t[:, nt // 2] = t[:, 0]                                               # an exact duplicate: the lower index must win
    qn, tn = N.unit_normals(rs, (B, nq)), N.unit_normals(rs, (B, nt))
    tn[:, nt // 2] = tn[:, 0]
    qc = np.array([nq if b == 0 else max(1, (nq * (B - b)) // B - b) for b in range(B)], np.int32)
    tc = np.array([nt if b == 0 else max(1, (nt * (B - b)) // B - b) for b in range(B)], np.int32)
    mask = None
    if masked:
        mask = rs.rand(B, nt) < 0.7
        mask[:, 0] = True
    return q, t, qn, tn, qc, tc, mask


@pytest.mark.parametrize("cos_min", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nt", [1, 257, 700])
@pytest.mark.parametrize("nq", [1, 255, 1025])
def test_gated_search_against_host_reference_bitwise(nq, nt, B, masked, cos_min):
    q, t, qn, tn, qc, tc, mask = search_case(nq, nt, B, masked)
    idx, d2 = ops.nearest_points(dev(q), dev(t), q_count=qc, t_count=tc, t_mask=mask, gate=(dev(qn), dev(tn), cos_min))
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    for b in range(B):
        m, k = int(qc[b]), int(tc[b])
        ri, rd = N.nearest_gated_f32(q[b, :m], t[b, :k], qn[b, :m], tn[b, :k], cos_min, None if mask is None else mask[b, :k])
        assert np.array_equal(idx[b, :m], ri), (b, np.nonzero(idx[b, :m] != ri)[0][:5])
        assert np.array_equal(d2[b, :m].view(np.int32), rd.view(np.int32)), b
        assert (idx[b, m:] == -1).all() and (d2[b, m:] == 0).all()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nt", [1, 257, 700])
@pytest.mark.parametrize("nq", [1, 255, 1025])
def test_open_gate_gives_the_ungated_bits(nq, nt, B, masked):
    q, t, qn, tn, qc, tc, mask = search_case(nq, nt, B, masked)
    plain = ops.nearest_points(dev(q), dev(t), q_count=qc, t_count=tc, t_mask=mask)
    gated, names = recorded(lambda: ops.nearest_points(dev(q), dev(t), q_count=qc, t_count=tc, t_mask=mask,
                                                       gate=(dev(qn), dev(tn), -math.inf)))
    assert "nearest_search_gated_kernel" in names and "nearest_search_kernel" not in names
    assert same(plain, gated)


# ------------------------------------------------------------------------------------------------ G4
def test_split_and_batching_invariance():
    nq, nt, cos_min = 300, 20011, 0.5
    rs = np.random.RandomState(4)
    q, t = rs.randn(1, nq, 3).astype(np.float32), rs.randn(1, nt, 3).astype(np.float32)
    qn, tn = N.unit_normals(rs, (1, nq)), N.unit_normals(rs, (1, nt))
    one = {c: ops.nearest_points(dev(q), dev(t), chunks=c, gate=(dev(qn), dev(tn), cos_min)) for c in (1, 2, 7, 79, 0)}
    Q, T, QN, TN = (np.concatenate([rs.randn(15, *a.shape[1:]).astype(np.float32), a]) for a in (q, t, qn, tn))
    sixteen = ops.nearest_points(dev(Q), dev(T), chunks=1, gate=(dev(QN), dev(TN), cos_min))
    ref = (sixteen[0][15:], sixteen[1][15:])
    for c, got in one.items():
        assert same(got, ref), c
    idx = ref[0].cpu().numpy()[0]
    assert (idx >= 0).mean() > 0.8 and (idx > 256).any()                   # not vacuous (about 5 % of the queries have a zero normal: no partner)
    ungated = ops.nearest_points(dev(q), dev(t))[0].cpu().numpy()[0]
    assert (ungated != idx).any()


# ------------------------------------------------------------------------------------------------ G5
def test_no_compatible_target():
    # the search: every target normal opposes every query normal; the last three queries lie beyond the count
    x, _ = N.bodies("small_ae.npz", 1)
    n = x.shape[1] - 1
    qn = np.tile(np.float32([0, 0, 1]), (1, n, 1))
    idx, d2 = ops.nearest_points(dev(x[:, :n] + np.float32(0.01)), dev(x), nt=n, q_count=[n - 3], gate=(dev(qn), dev(-qn), 0.5))
    assert (idx[0, :n - 3] == -1).all() and torch.isinf(d2[0, :n - 3]).all() and (d2[0, :n - 3] > 0).all()
    assert (idx[0, n - 3:] == -1).all() and (d2[0, n - 3:] == 0).all()
    # chamfer: a plane patch whose vertex normals are all exactly +z, a scan that says -z everywhere -> no pair in either
    # direction, the loss is trunc^2 (+ w trunc^2) and the gradient exactly zero
    plane = np.zeros((1, 10, 3), np.float32)
    plane[0, :9, :2] = np.stack(np.meshgrid(np.arange(3.0), np.arange(3.0), indexing="ij"), -1).reshape(-1, 2)
    pf = np.array([[0, 3, 1], [1, 3, 4], [1, 4, 2], [2, 4, 5], [3, 6, 4], [4, 6, 7], [4, 7, 5], [5, 7, 8]])
    pd = dev(plane).requires_grad_(True)
    assert np.array_equal(scan.vertex_normals(pd, pf).cpu().numpy()[0], np.tile(np.float32([0, 0, 1]), (9, 1)))
    sb = scan.ScanBatch(plane[:, :9] + np.float32([0.1, 0.1, 0.05]), DEV, normals=np.tile([0.0, 0.0, -1.0], (1, 9, 1)))
    trunc, w = 0.25, 0.5                                                   # exact in fp32, and so are trunc^2 and 1.5 trunc^2
    m = {}
    loss = scan.chamfer(pd, sb, trunc=trunc, w_model_to_scan=w, matches=m, normal_angle=60, normal_faces=pf)
    loss.sum().backward()
    assert (m["idx_sm"] == -1).all() and torch.isinf(m["d2_sm"]).all()
    assert (m["idx_ms"][:, :9] == -1).all() and torch.isinf(m["d2_ms"][:, :9]).all()
    assert float(loss[0]) == trunc ** 2 * (1 + w)
    assert (pd.grad == 0).all()
    assert float(scan.chamfer(pd, sb, trunc=trunc, normal_angle=60, normal_faces=pf)[0]) == trunc ** 2


# ------------------------------------------------------------------------------------------------ G6
def slab(k=12, h=0.02):
    """A closed box [0, 1] x [0, 1] x [0, h]: top and bottom regular k x k grids, four side strips, faces oriented outward.
    Vertices 0 .. k*k - 1 are the top (z = h), k*k .. 2 k*k - 1 the bottom (z = 0), plus the dummy row."""
    g = np.linspace(0.0, 1.0, k)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    top = np.concatenate([xy, np.full((k * k, 1), h)], 1)
    bot = np.concatenate([xy, np.zeros((k * k, 1))], 1)
    v = np.concatenate([top, bot, np.zeros((1, 3))]).astype(np.float32)
    faces = []
    for i in range(k - 1):
        for j in range(k - 1):
            a, b, c, d = i * k + j, (i + 1) * k + j, (i + 1) * k + j + 1, i * k + j + 1      # a -> b: +x, a -> d: +y
            faces += [[a, b, c], [a, c, d]]                                                 # top: counter-clockwise from +z
            A, Bq, Cq, D = (u + k * k for u in (a, b, c, d))
            faces += [[A, Cq, Bq], [A, D, Cq]]                                              # bottom: from -z
    ring = [i * k for i in range(k)] + [(k - 1) * k + j for j in range(1, k)] + [i * k + k - 1 for i in range(k - 2, -1, -1)] + \
           [j for j in range(k - 2, 0, -1)]                                                 # the boundary, counter-clockwise from +z
    for a, b in zip(ring, ring[1:] + ring[:1]):
        faces += [[a + k * k, b + k * k, b], [a + k * k, b, a]]                             # the side wall, outward
    return v, np.asarray(faces, np.int64), k * k


def test_slab_faces_are_outward():
    v, f, kk = slab()
    nrm = scan.vertex_normals(dev(v[None]), f).cpu().numpy()[0]
    inner = np.array([i * 12 + j for i in range(1, 11) for j in range(1, 11)])
    assert np.array_equal(nrm[inner], np.tile(np.float32([0, 0, 1]), (100, 1)))
    assert np.array_equal(nrm[inner + kk], np.tile(np.float32([0, 0, -1]), (100, 1)))
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    centre = np.array([0.5, 0.5, 0.01])
    assert (np.einsum("ij,ij->i", np.cross(b - a, c - a), (a + b + c) / 3 - centre) > 0).all()


def test_thin_slab_needs_the_gate():
    """Fails without the feature: the scan of the TOP face, 0.75 h below it, lies nearer the bottom."""
    h = 0.02
    v, f, kk = slab(h=h)
    x = dev(v[None]).requires_grad_(True)
    pts = v[None, :kk].copy()
    pts[:, :, 2] -= np.float32(0.75 * h)
    sb = scan.ScanBatch(pts, DEV, normals=np.tile([0.0, 0.0, 1.0], (1, kk, 1)))
    trunc = 0.5
    m = {}
    plain = scan.chamfer(x, sb, trunc=trunc, matches=m)
    assert ((m["idx_sm"] >= kk) & (m["idx_sm"] < 2 * kk)).all()            # every match is a bottom vertex
    m = {}
    loss = scan.chamfer(x, sb, trunc=trunc, matches=m, normal_angle=60, normal_faces=f)
    idx = m["idx_sm"].cpu().numpy()[0]
    assert ((idx >= 0) & (idx < kk)).all() and np.array_equal(idx, np.arange(kk))          # every match is a top vertex: its own
    d = (v[:kk, 2].astype(np.float32) - pts[0, :, 2]).astype(np.float64)   # the fp32 differences the kernel forms
    want = float(np.mean(d * d))
    rel = abs(float(loss[0]) - want) / want
    print("slab: gated loss %.9g, mean((0.75 h)^2) from the fp32 differences %.9g (rel %.2e); ungated loss %.9g"
          % (float(loss[0]), want, rel, float(plain[0])))
    assert rel <= 1.01 * 2.0 ** -23                                        # dz * dz rounded to fp32 (2^-24) and the fp64 mean rounded to fp32 (2^-24)
    # the fp32 roundings of h, 0.75 h and their difference move dz by at most 2^-24 (h + 0.75 h + 0.25 h) = 2.7 x 2^-24 of 0.75 h
    assert abs(want / (0.75 * h) ** 2 - 1) <= 6 * 2.0 ** -24
    assert float(plain[0]) < 0.2 * float(loss[0])                          # the ungated loss is the (0.25 h)^2 of the wrong side
    loss.sum().backward()
    g = x.grad.cpu().numpy()[0]
    assert (g[:kk, 2] > 0).all() and (g[kk:] == 0).all()                   # x_i - s_j points up; nothing pulls the bottom


# ------------------------------------------------------------------------------------------------ G7, G8
@functools.lru_cache(maxsize=None)
def fit_setup():
    m, z0, z_kps, dummy, scans, x_star, n = semantic_setup()
    h = load_hierarchy(os.path.join(GOLD, "semantic.npz"))
    faces = np.asarray(h.faces, np.int64)
    B = len(scans)
    clouds = [scans.points[b, :int(scans.host_counts[b])].cpu().numpy() for b in range(B)]
    rs = np.random.RandomState(5)
    normals = [N.unit_normals(rs, (c.shape[0],)) for c in clouds]
    with_n = scan.ScanBatch(clouds, DEV, normals=normals)
    return m, z0, z_kps, dummy, scans, with_n, x_star, n, faces


def three_entry_points(scans, **gate):
    m, z0, z_kps, dummy, _, _, x_star, n, _ = fit_setup()
    trunc = 0.5 * float(x_star[:, :n].abs().max())
    x = (x_star.detach() * 1.02).requires_grad_(True)
    loss = scan.chamfer(x, scans, trunc=trunc, w_model_to_scan=0.5, **gate)
    loss.sum().backward()
    pose, aligned, log = scan.align(x_star, scans, mode="similarity", iters=4, trunc=trunc, **gate)
    fit = editing.fit_scan(m, z0, z_kps, scans, parts=PARTS, steps=5, lr=1e-2, w_model_to_scan=0.5, trunc=trunc, dummy=dummy, **gate)
    return [loss.detach(), x.grad, pose.packed, pose.scale, aligned.points, log, *fit]


def test_off_means_off():
    _, _, _, _, scans, with_n, _, _, _ = fit_setup()
    base = three_entry_points(scans)
    got, names = recorded(lambda: three_entry_points(with_n))
    assert same(base, got)
    assert not (names & NEW_KERNELS), sorted(names)
    assert "nearest_search_kernel" in names


def test_angle_180_equals_no_gate_bitwise():
    _, _, _, _, scans, with_n, _, _, faces = fit_setup()
    base = three_entry_points(scans)
    got, names = recorded(lambda: three_entry_points(with_n, normal_angle=180, normal_faces=faces))
    assert NEW_KERNELS <= names and "nearest_search_kernel" not in names, sorted(names)
    assert same(base, got)
    gated = three_entry_points(with_n, normal_angle=60, normal_faces=faces)
    assert not same(base[:1], gated[:1])                                   # random scan normals at 60 degrees do change the loss


# ------------------------------------------------------------------------------------------------ G9
def test_pose_carries_normals():
    rs = np.random.RandomState(9)
    B, M = 3, 50
    clouds = [rs.randn(M - 7 * b, 3).astype(np.float32) for b in range(B)]
    normals = [N.unit_normals(rs, (c.shape[0],)) for c in clouds]
    sb = scan.ScanBatch(clouds, DEV, normals=normals)
    qr = np.linalg.qr(rs.randn(B, 3, 3))[0]
    qr *= np.sign(np.linalg.det(qr))[:, None, None]
    sc = np.array([0.5, 1.0, 3.7])
    pose = scan.Pose(torch.from_numpy((qr * sc[:, None, None]).astype(np.float32)).to(DEV), torch.from_numpy(rs.randn(B, 3).astype(np.float32)).to(DEV),
                     torch.from_numpy(sc.astype(np.float32)).to(DEV))

    def check(p, got):
        R = p.A.double().cpu().numpy() / p.scale.double().cpu().numpy()[:, None, None]
        want = np.einsum("brc,bmc->bmr", R, sb.normals.double().cpu().numpy())
        err = np.abs(got.double().cpu().numpy() - want).max()
        assert err <= 4 * 2.0 ** -23, err
        for b in range(B):
            assert (got[b, clouds[b].shape[0]:] == 0).all()

    aligned = pose.apply(sb)
    check(pose, aligned.normals)
    assert pose.apply(scan.ScanBatch(clouds, DEV)).normals is None
    # pose_update: from the ORIGINAL normals under the composed pose, not chained
    x = torch.from_numpy(rs.randn(B, M, 3).astype(np.float32)).to(DEV)
    m = {}
    scan.chamfer(x, aligned, n=M, trunc=10.0, w_model_to_scan=0.5, matches=m)
    aligned.normals.fill_(7.0)                                             # a chained update would carry this along
    scan.pose_update(pose, sb, aligned, m, "similarity")
    check(pose, aligned.normals)
    assert same([aligned.normals], [pose.apply(sb).normals])


def test_gated_align_batch_of_16_against_one_body():
    v, f = N.template("small_ae.npz")
    n = v.shape[0]
    x = scan_ref.model_points(v, 16, seed=2)
    xd = dev(x)
    nrm = scan.vertex_normals(xd, f).cpu().numpy()
    rs = np.random.RandomState(3)
    clouds, normals = [], []
    for b in range(16):
        pick = rs.randint(0, n, size=300 - b)
        clouds.append((x[b, :n][pick] * np.float32(1.1) + np.float32([0.02, -0.01, 0.03])).astype(np.float32))
        normals.append(nrm[b][pick])
    sb = scan.ScanBatch(clouds, DEV, normals=normals)
    trunc = 0.3 * float(np.abs(x).max())
    pose, aligned, log = scan.align(xd, sb, iters=5, trunc=trunc, normal_angle=60, normal_faces=f)
    assert torch.isfinite(log).all() and torch.isfinite(pose.packed).all()
    assert (aligned.normals.norm(dim=2) > 0.5).float().mean() > 0.9        # the aligned batch does carry rotated unit normals
    for b in (0, 9, 15):
        s = slice(b, b + 1)
        p1, a1, l1 = scan.align(xd[s], sb.select(s), iters=5, trunc=trunc, normal_angle=60, normal_faces=f)
        assert same([p1.packed, p1.scale, a1.points, a1.normals, l1], [pose.packed[s], pose.scale[s], aligned.points[s], aligned.normals[s], log[:, s]]), b


# ------------------------------------------------------------------------------------------------ G10
def test_argument_errors():
    v, f, kk = slab(k=4)
    x = dev(v[None])
    pts = v[None, :kk]
    nrm = np.tile([0.0, 0.0, 1.0], (1, kk, 1))
    with_n, without = scan.ScanBatch(pts, DEV, normals=nrm), scan.ScanBatch(pts, DEV)
    for fn in (scan.chamfer, scan.align):
        with pytest.raises(ValueError, match="scan normals"):
            fn(x, without, trunc=1.0, normal_angle=60, normal_faces=f)
        with pytest.raises(ValueError, match="normal_faces"):
            fn(x, with_n, trunc=1.0, normal_angle=60)
        with pytest.raises(ValueError, match="trunc"):
            fn(x, with_n, normal_angle=60, normal_faces=f)
        for bad in (0, -1, 180.5, float("nan")):
            with pytest.raises(ValueError, match="normal_angle"):
                fn(x, with_n, trunc=1.0, normal_angle=bad, normal_faces=f)
    with pytest.raises(ValueError, match="not built"):
        scan.chamfer(x, with_n, trunc=1.0, faces=f, normal_angle=60, normal_faces=f)
    m, z0, z_kps, dummy, _, fit_n, _, _, faces = fit_setup()
    with pytest.raises(ValueError, match="not built"):
        editing.fit_scan(m, z0, z_kps, fit_n, parts=PARTS, steps=1, trunc=1.0, dummy=dummy, faces=faces, normal_angle=60, normal_faces=faces)
    with pytest.raises(ValueError, match="not built"):
        editing.register_scan(m, z0, z_kps, fit_n, parts=PARTS, steps=1, align_iters=1, trunc=1.0, dummy=dummy, faces=faces, normal_angle=60,
                              normal_faces=faces)
    with pytest.raises(ValueError, match="trunc"):
        editing.register_scan(m, z0, z_kps, fit_n, parts=PARTS, steps=1, align_iters=1, dummy=dummy, normal_angle=60, normal_faces=faces)
