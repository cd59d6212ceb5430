"""Cloud normals on the GPU (sh_cloud_normals, scan.estimate_normals, ScanBatch(normals="estimate")) against the host reference
of tests/cloud_normals_ref.py: neighbourhoods bitwise, normals within the derived bound, ragged and degenerate bodies, ties,
determinism over batch, padding and launch shape, the sign rules, the plumbing into the gated Chamfer loss, and the argument
checks of the C ABI."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, ops, scan
from tests import cloud_normals_ref as R
from tests import normals_ref as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INPUTS = {"small63": (("small_ae.npz", 63, 5),), "small1000": (("small_ae.npz", 1000, 5),),
          "template5000x2": (("template6890.npz", 5000, 5), ("template6890.npz", 5000, 6))}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(out):
    return tuple(t.cpu().numpy() for t in out)


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


def clouds_of(key):
    return np.stack([R.samples(*c)[0] for c in INPUTS[key]])


@functools.lru_cache(maxsize=None)
def gpu_run(key, k):
    """(nrm, var, r2, cnt) of one input at one k, on the host; computed once, shared by the tests, read-only."""
    return host(scan.estimate_normals(dev(clouds_of(key)), k=k))


def check_normals(what, got, cnt, S1, S2, s=None, view=None, min_compared=1.0):
    """Item 2: the angle to the reference within R.angle_bound on every point whose bound says anything (below 1e-3 rad; on the
    surface samples that is every point - no point is left out for a small gap), var within 4 2^-24 var + 1e-12, the unknown
    points the same.  -> the largest error over the bound."""
    nrm, var = got
    ref_n, ref_var, gap, spread, _ = R.finish(cnt, S1, S2, s, view)
    known = np.abs(ref_n).sum(1) > 0
    with np.errstate(divide="ignore"):
        bound = np.where(known, R.angle_bound(cnt, np.where(known, gap, 1.0)), np.inf)
    cmp = known & (bound <= 1e-3) & (spread <= R.SPREAD_MAX)
    left_out = 1.0 - cmp.sum() / max(int(known.sum()), 1)
    assert (np.abs(nrm[~known]).sum(1) == 0).all() and (var[~known] == 0).all(), what
    assert (np.abs(nrm[cmp]).sum(1) > 0).all(), what
    ang = R.unsigned_angle(nrm[cmp], ref_n[cmp])
    worst = float((ang / bound[cmp]).max()) if cmp.any() else 0.0
    clear = cmp.copy()                                                      # the sign too, where the leading component is clear
    top = np.sort(np.abs(ref_n.astype(np.float64)), 1)
    clear &= top[:, 2] - top[:, 1] > 1e-5
    print("%s: %d of %d known points compared (%.4f left out), largest angle error over the bound %.3e, smallest gap %.2e"
          % (what, cmp.sum(), known.sum(), left_out, worst, gap[cmp].min() if cmp.any() else np.nan))
    assert left_out <= 1.0 - min_compared + 0.01, what
    assert worst <= 1.0, what
    assert (N.angle(nrm[clear], ref_n[clear]) <= bound[clear]).all(), what
    assert (np.abs(var[cmp].astype(np.float64) - ref_var[cmp]) <= 4 * 2.0 ** -24 * ref_var[cmp] + 1e-12).all(), what
    assert np.abs(np.linalg.norm(nrm[known].astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22 if known.any() else True
    return worst


# ------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("key", list(INPUTS))
def test_neighbourhoods_are_exact(key, k):
    nrm, var, r2, cnt = gpu_run(key, k)
    for b, case in enumerate(INPUTS[key]):
        rr, rc, _, _ = R.reference(*case)[k]
        assert np.array_equal(r2[b].view(np.int32), rr.view(np.int32)), (key, k, b, np.nonzero(r2[b] != rr)[0][:5])
        assert np.array_equal(cnt[b], rc), (key, k, b)
        assert (cnt[b] >= min(k, case[1])).all()


@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("key", list(INPUTS))
def test_normals_against_the_reference(key, k):
    """Largest angle error over the bound 4 2^-24 + 384 (cnt + 16) 2^-53 / gap, every point compared (none left out)."""
    nrm, var, r2, cnt = gpu_run(key, k)
    for b, case in enumerate(INPUTS[key]):
        rr, rc, S1, S2 = R.reference(*case)[k]
        check_normals("%s k=%d body %d" % (key, k, b), (nrm[b], var[b]), rc, S1, S2)


# ------------------------------------------------------------------------------------------------ 3
def test_ragged_batch_and_degenerate_bodies():
    src = R.samples("small_ae.npz", 1000)[0]
    counts = np.array([0, 2, 5, 1000], np.int32)
    s = np.full((4, 1000, 3), np.nan, np.float32)                          # the padding is never read as points
    for b, m in enumerate(counts):
        s[b, :m] = src[:m]
    nrm, var, r2, cnt = host(scan.estimate_normals(dev(s), k=16, counts=counts))
    for b, m in enumerate(counts):
        assert (nrm[b, m:] == 0).all() and (var[b, m:] == 0).all() and (r2[b, m:] == 0).all() and (cnt[b, m:] == 0).all(), b
    assert (nrm[:2] == 0).all() and (var[:2] == 0).all() and (r2[0] == 0).all() and (cnt[0] == 0).all()
    assert (cnt[1, :2] == 2).all() and np.array_equal(r2[1, :2], np.repeat(R.d2_f32(src[0], src[1]), 2))
    for b in (2, 3):
        m = int(counts[b])
        rr, rc, S1, S2 = R.neighbourhoods(src[:m], (16,))[16] if b == 2 else R.reference("small_ae.npz", 1000)[16]
        assert np.array_equal(r2[b, :m].view(np.int32), rr.view(np.int32)) and np.array_equal(cnt[b, :m], rc)
        check_normals("ragged body %d" % b, (nrm[b, :m], var[b, :m]), rc, S1, S2)
    assert (cnt[2, :5] == 5).all()                                          # k_eff = 5: every point is every point's neighbour


# ------------------------------------------------------------------------------------------------ 4
def test_ties_duplicates_collinear_and_planar():
    lat = R.lattice()
    for k in (8, 16):
        nrm, var, r2, cnt = (a[0] for a in host(scan.estimate_normals(dev(lat[None]), k=k)))
        rr, rc, S1, S2 = R.neighbourhoods(lat, (k,))[k]
        assert (cnt > k).any() and cnt[14] >= k
        assert np.array_equal(r2.view(np.int32), rr.view(np.int32)) and np.array_equal(cnt, rc)
        ref_n, _, gap, _, lam = R.finish(rc, S1, S2)
        # a symmetric lattice neighbourhood can have l0 = l1: its normal is anyone's; the others are held to the bound
        check_normals("lattice k=%d" % k, (nrm, var), rc, S1, S2, min_compared=0.25)
    nrm, var, r2, cnt = host(scan.estimate_normals(dev(R.collinear()[None]), k=8))
    assert (nrm == 0).all() and (var == 0).all() and (cnt >= 8).all()
    pl = R.planar()
    nrm, var, r2, cnt = (a[0] for a in host(scan.estimate_normals(dev(pl[None]), k=16)))
    rr, rc, S1, S2 = R.neighbourhoods(pl, (16,))[16]
    check_normals("planar", (nrm, var), rc, S1, S2)
    assert (np.abs(nrm[:, 2]) >= 1 - 2.0 ** -22).all() and (var <= 1e-12).all()


# ------------------------------------------------------------------------------------------------ 5
def test_determinism_batch_padding_and_launch_shape():
    src = R.samples("small_ae.npz", 1000)[0]
    alone = host(scan.estimate_normals(dev(src[None]), k=16))
    assert same(alone, host(scan.estimate_normals(dev(src[None]), k=16)))
    assert same(alone, gpu_run("small1000", 16))
    rs = np.random.RandomState(4)
    s = rs.rand(16, 1200, 3).astype(np.float32)                            # the same body as one of 16, in a wider padded tensor
    counts = rs.randint(1, 1200, 16).astype(np.int32)
    s[7, :1000], counts[7] = src, 1000
    batch = host(scan.estimate_normals(dev(s), k=16, counts=counts))
    assert same([a[0] for a in alone], [a[7, :1000] for a in batch])
    # 512 small bodies: several queries per thread (the other instantiation of every list capacity) - the same bits again
    small = R.samples("small_ae.npz", 63)[0]
    s = rs.rand(512, 64, 3).astype(np.float32)
    counts = rs.randint(1, 65, 512).astype(np.int32)
    s[300, :63], counts[300] = small, 63
    for k in (8, 16, 32):
        wide = host(scan.estimate_normals(dev(s), k=k, counts=counts))
        assert same([a[0] for a in gpu_run("small63", k)], [a[300, :63] for a in wide]), k


# ------------------------------------------------------------------------------------------------ 6
def test_sign_rules():
    s = clouds_of("small1000")
    m = s.shape[1]
    free = gpu_run("small1000", 16)
    n0 = free[0][0]
    known = np.abs(n0).sum(1) > 0
    assert known.all() and (n0.max(1) == np.abs(n0).max(1)).all()           # the largest-magnitude component is positive
    per_body = np.float32([[0.3, 2.0, 1.5]])
    per_point = np.where((np.arange(m) % 2 == 0)[:, None], np.float32([2.0, 0.1, 0.4]), np.float32([-1.5, 0.2, -2.0])).astype(np.float32)[None]
    for view in (per_body, per_point):
        got = host(scan.estimate_normals(dev(s), k=16, viewpoints=dev(view)))
        assert same(got[1:], free[1:])
        n = got[0][0]
        v = np.broadcast_to(view.reshape(-1, 3), n.shape)
        _, dot = R.orient(n, s[0], v)
        assert (dot >= 0).all()
        flipped = (n != n0).any(1)
        assert flipped.any() and not flipped.all()
        assert np.array_equal(np.where(flipped[:, None], -n, n).view(np.int32), n0.view(np.int32))     # up to sign: the unoriented bits
        assert np.array_equal(n, R.orient(n0, s[0], v)[0])
    # host viewpoints in the three accepted shapes give what the device tensors give
    a = host(scan.estimate_normals(dev(s), k=16, viewpoints=per_body[0]))
    b = host(scan.estimate_normals(dev(s), k=16, viewpoints=[per_point[0]]))
    assert same(a, host(scan.estimate_normals(dev(s), k=16, viewpoints=dev(per_body)))) and same(b, got)


# ------------------------------------------------------------------------------------------------ 7
def plumbing_case():
    x, f = N.bodies("small_ae.npz", 2)
    n = x.shape[1] - 1
    from tests.surface_gated_ref import sample_surface_faces
    clouds = [sample_surface_faces(x[b, :n], f, m, seed=20 + b, sigma=0.002)[0] for b, m in enumerate((700, 1000))]
    centre = x[:, :n].mean(1)
    views = [np.where((np.arange(len(c)) % 2 == 0)[:, None], centre[b] + np.float32([0, 0, 3]), centre[b] + np.float32([0, 0, -3])).astype(np.float32)
             for b, c in enumerate(clouds)]
    return x, f, n, clouds, views


def test_scanbatch_estimate_feeds_the_gated_chamfer():
    x, f, n, clouds, views = plumbing_case()
    batch = scan.ScanBatch(clouds, DEV, normals="estimate", normal_k=16, viewpoints=views)
    assert batch.normals.dtype == torch.float32 and tuple(batch.normals.shape) == tuple(batch.points.shape)
    vd = dev(scan.pack_viewpoints(views, batch.host_counts, batch.points.shape[1]))
    assert torch.equal(batch.normals.view(torch.int32), scan.estimate_normals(batch.points, 16, vd, batch.counts)[0].view(torch.int32))
    assert torch.equal(batch.normals.view(torch.int32), scan.estimate_normals(batch, 16, views)[0].view(torch.int32))
    nh = batch.normals.cpu().numpy()
    given = scan.ScanBatch(clouds, DEV, normals=[nh[b, :m] for b, m in enumerate(batch.host_counts)])
    out = []
    for sb in (batch, given):
        xd = dev(x).requires_grad_(True)
        loss = scan.chamfer(xd, sb, normal_angle=60, trunc=0.1, normal_faces=f, w_model_to_scan=1.0)
        loss.sum().backward()
        out.append((loss.detach().cpu().numpy(), xd.grad.cpu().numpy()))
    assert same(out[0], out[1]) and np.isfinite(out[0][0]).all() and np.abs(out[0][1]).max() > 0
    plain = scan.ScanBatch(clouds, DEV)                                     # off means off: no estimate unless asked for
    assert plain.normals is None


def test_scanbatch_estimate_after_the_morton_sort():
    x, f, n, clouds, views = plumbing_case()
    plain = scan.ScanBatch(clouds, DEV, normals="estimate", normal_k=16, viewpoints=views)
    srt = scan.ScanBatch(clouds, DEV, order="morton", normals="estimate", normal_k=16, viewpoints=views)
    u = host(scan.estimate_normals(plain, 16))
    t = host(scan.estimate_normals(srt, 16))
    pts, nrm = srt.points.cpu().numpy(), srt.normals.cpu().numpy()
    for b, m in enumerate(srt.host_counts):
        perm = srt.perm[b, :m]
        assert np.array_equal(pts[b, :m], clouds[b][perm])
        assert np.array_equal(t[2][b, :m].view(np.int32), u[2][b, :m][perm].view(np.int32)) and np.array_equal(t[3][b, :m], u[3][b, :m][perm])
        rr, rc, S1, S2 = R.neighbourhoods(pts[b, :m], (16,))[16]
        assert np.array_equal(t[2][b, :m].view(np.int32), rr.view(np.int32)) and np.array_equal(t[3][b, :m], rc)
        check_normals("morton body %d" % b, (nrm[b, :m], t[1][b, :m]), rc, S1, S2, pts[b, :m], views[b][perm])
        _, dot = R.orient(nrm[b, :m], pts[b, :m], views[b][perm])          # the per-point viewpoints went with their points
        assert (dot >= 0).all()
        assert (nrm[b, m:] == 0).all()


# ------------------------------------------------------------------------------------------------ 8
def test_cabi_validates_before_the_device():
    lib = _lib.load()
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)                 # `some` is never dereferenced: every call fails its checks
    for k in (2, 65):
        assert lib.sh_cloud_normals(some, 30, 10, null, 1, k, null, 0, 0, some, null, some, null, null, 0, null) == -1
        assert b"k = %d" % k in lib.sh_last_error()
    assert lib.sh_cloud_normals(some, 30, 10, null, 1, 16, null, 0, 0, null, null, some, null, null, 0, null) == -1
    assert b"null pointer" in lib.sh_last_error()
    assert lib.sh_cloud_normals(null, 30, 10, null, 1, 16, null, 0, 0, some, null, some, null, null, 0, null) == -1
    assert lib.sh_cloud_normals(some, 30, -1, null, 1, 16, null, 0, 0, some, null, some, null, null, 0, null) == -1
    assert b"negative" in lib.sh_last_error()
    assert lib.sh_cloud_normals(some, 29, 10, null, 1, 16, null, 0, 0, some, null, some, null, null, 0, null) == -1
    assert lib.sh_cloud_normals(some, 30, 10, null, 1, 16, some, 3, 2, some, null, some, null, null, 0, null) == -1
    assert b"viewpoint" in lib.sh_last_error()
    assert lib.sh_cloud_normals(some, 30, 10, null, 1, 16, null, 0, 0, some, null, null, null, null, 0, null) == -3     # no r2, no workspace
    assert lib.sh_cloud_normals(some, 30, 10, null, 0, 16, null, 0, 0, some, null, some, null, null, 0, null) == 0      # B == 0: nothing to do
    with pytest.raises(ValueError):
        ops.cloud_normals(torch.zeros((1, 8, 3), device=DEV), k=2)
    with pytest.raises(ValueError):
        ops.cloud_normals(torch.zeros((1, 8, 3), device=DEV), view=torch.zeros((2, 3), device=DEV))
    with pytest.raises(RuntimeError):
        scan.estimate_normals(torch.zeros((1, 8, 3)), k=16)                # no CPU path
