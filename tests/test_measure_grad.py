"""Gradients of the body measurements (sh_measure_girth_bwd, sh_bone_length_bwd, sh_joint_regress_bwd through
measure.girths / bone_lengths / joints) against float64 torch autograd of the CPU oracle."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from semantichuman_amd import constants as C
from semantichuman_amd import measure

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def dev():
    return torch.device("cuda:0")


def rings_of(g):
    n = int(g["n_planes"])
    return [g["factor_%d" % i] for i in range(n)], [g["epi_%d" % i] for i in range(n)]


def close(got, ref, what):
    gmax = float(ref.abs().max())
    err = float((got.double().cpu() - ref).abs().max())
    assert err <= 1e-5 * gmax + 1e-7, "%s: max |d| %.3g, max |g| %.3g" % (what, err, gmax)


def safe_girths(v, fac, epi):
    """float64 girths whose zero-length segments have gradient 0 (the oracle's sqrt would give NaN there)."""
    out = []
    for f, e in zip(fac, epi):
        f = torch.as_tensor(np.asarray(f, dtype=np.float64).reshape(-1, 1))
        e = torch.as_tensor(np.asarray(e, dtype=np.int64))
        q = v[e[:, 0]] * (1 - f) + v[e[:, 1]] * f
        d = q - q.roll(-1, 0)
        s = (d * d).sum(1)
        nz = s > 0
        out.append(torch.where(nz, torch.sqrt(torch.where(nz, s, torch.ones_like(s))), torch.zeros_like(s)).sum())
    return torch.stack(out)


def meshes(verts, B, seed, rows_extra=1):
    g = torch.Generator().manual_seed(seed)
    v = torch.as_tensor(verts, dtype=torch.float32)[None].repeat(B, 1, 1)
    v = v * (1 + 0.05 * torch.randn((B, 1, 3), generator=g)) + 0.01 * torch.randn(v.shape, generator=g)
    return torch.cat([v, torch.zeros((B, rows_extra, 3))], 1)                  # + the dummy row


def girth_case(v32, fac, epi, seed, oracle=ref_cpu.girths):
    rings = measure.GirthRings(fac, epi, dev())
    vd = v32.to(dev()).requires_grad_(True)
    gi = measure.girths(vd, rings)
    w = torch.randn(gi.shape, generator=torch.Generator().manual_seed(seed))
    (gi * w.to(dev())).sum().backward()
    v64 = v32.double().requires_grad_(True)
    ref = torch.stack([oracle(v64[b], fac, epi) for b in range(v64.shape[0])])
    (ref * w.double()).sum().backward()
    close(gi.detach(), ref.detach(), "girth")
    close(vd.grad, v64.grad, "girth gradient")
    return rings, vd, w


@pytest.mark.parametrize("B", [1, 5, 64])
def test_girth_gradient_golden_rings(B):
    g = np.load(os.path.join(GOLD, "measure.npz"))
    fac, epi = rings_of(g)
    v = meshes(g["verts"], B, seed=B)
    rings, vd, w = girth_case(v, fac, epi, seed=100 + B)
    # untouched rows (the dummy row among them) are exactly 0
    touched = np.zeros(v.shape[1], bool)
    for e in epi:
        touched[np.asarray(e).reshape(-1)] = True
    gv = vd.grad.cpu()
    assert not touched[-1] and torch.all(gv[:, ~torch.from_numpy(touched)] == 0)
    # deterministic: two calls, the same bits
    from semantichuman_amd import ops
    g1 = ops.measure_girth_bwd(vd.detach(), rings, w.to(dev()))
    g2 = ops.measure_girth_bwd(vd.detach(), rings, w.to(dev()))
    assert torch.equal(g1, g2) and torch.equal(g1, vd.grad)


def test_girth_gradient_synthetic_rings_6890():
    t = np.load(os.path.join(GOLD, "template6890.npz"))
    verts = t["verts"]
    rng = np.random.default_rng(3)
    fac, epi = [], []
    for n in (3, 17, 80, 150, 2):
        epi.append(rng.integers(0, verts.shape[0], size=(n, 2)))
        fac.append(rng.random((n, 1)).astype(np.float32))
    v = meshes(verts, 64, seed=9)
    girth_case(v, fac, epi, seed=11)


def test_girth_zero_length_segments_and_small_rings():
    g = np.load(os.path.join(GOLD, "measure.npz"))
    v = meshes(g["verts"], 4, seed=5)
    # n == 1 (girth 0, gradient 0), n == 2 (the segment twice), a repeated point (zero-length segment), a point with a == b
    fac = [np.float32([0.5]), np.float32([0.25, 0.75]), np.float32([0.1, 0.1, 0.6, 0.3]), np.float32([0.5, 0.2, 0.9])]
    epi = [np.array([[4, 5]]), np.array([[0, 1], [2, 3]]), np.array([[6, 7], [6, 7], [8, 9], [7, 11]]),
           np.array([[13, 13], [1, 19], [19, 12]])]
    rings, vd, w = girth_case(v, fac, epi, seed=3, oracle=safe_girths)
    gi = measure.girths(vd.detach(), rings)
    assert torch.all(gi[:, 0] == 0)
    # the one-point ring alone: gradient exactly 0
    r1 = measure.GirthRings([np.float32([0.5])], [np.array([[4, 5]])], dev())
    x = v.to(dev()).requires_grad_(True)
    measure.girths(x, r1).sum().backward()
    assert torch.all(x.grad == 0)


@pytest.mark.parametrize("skl", ["SKL_LIST[1:]", "NEWSKL_LIST"])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_bone_length_gradient(skl, B):
    bl = C.SKL_LIST[1:] if skl == "SKL_LIST[1:]" else C.NEWSKL_LIST
    g = np.load(os.path.join(GOLD, "measure.npz"))
    k0 = torch.from_numpy(g["kps"])
    gen = torch.Generator().manual_seed(B)
    kps = k0[torch.arange(B) % k0.shape[0]] + 0.01 * torch.randn((B,) + k0.shape[1:], generator=gen)
    kps = kps.float().contiguous()
    bones = measure.Bones(bl, dev())
    kd = kps.to(dev()).requires_grad_(True)
    ln = measure.bone_lengths(kd, bones)
    w = torch.randn(ln.shape, generator=gen)
    (ln * w.to(dev())).sum().backward()
    k64 = kps.double().requires_grad_(True)
    ref = torch.stack([ref_cpu.bone_lengths(k64[b], bl) for b in range(B)])
    (ref * w.double()).sum().backward()
    close(ln.detach(), ref.detach(), "length")
    close(kd.grad, k64.grad, "length gradient")
    used = sorted({j for s in bl for j in s})
    unused = [j for j in range(kps.shape[1]) if j not in used]
    assert torch.all(kd.grad[:, unused] == 0)
    from semantichuman_amd import ops
    assert torch.equal(ops.bone_length_bwd(kd.detach(), bones, w.to(dev())), ops.bone_length_bwd(kd.detach(), bones, w.to(dev())))


def test_zero_length_bone_has_zero_gradient():
    bl = [[0, 1], [2, 3, 4], [5, 6]]
    kps = torch.randn((3, 7, 3))
    kps[:, 1] = kps[:, 0]                                   # bone 0: zero length
    kps[:, 3] = kps[:, 2]                                   # bone 1: the tail midpoint (x + x) / 2 == x on the head
    kps[:, 4] = kps[:, 2]
    kd = kps.to(dev()).contiguous().requires_grad_(True)
    ln = measure.bone_lengths(kd, bl)
    assert torch.all(ln[:, :2] == 0)
    ln.sum().backward()
    assert torch.all(kd.grad[:, :5] == 0)
    u = (kps[:, 5] - kps[:, 6]) / (kps[:, 5] - kps[:, 6]).norm(dim=1, keepdim=True)
    torch.testing.assert_close(kd.grad[:, 5].cpu(), u, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("B", [1, 5, 64])
def test_joint_regression_gradient(B):
    s = np.load(os.path.join(GOLD, "semantic.npz"))
    J = torch.from_numpy(s["J_regressor"].astype(np.float32))
    x = meshes(s["verts"], B, seed=20 + B)
    Jd = J.to(dev()).contiguous()
    xd = x.to(dev()).requires_grad_(True)
    kps = measure.joints(xd, Jd)
    w = torch.randn(kps.shape, generator=torch.Generator().manual_seed(B))
    (kps * w.to(dev())).sum().backward()
    x64 = x.double().requires_grad_(True)
    ref = torch.matmul(J.double(), x64[:, :J.shape[1]])
    (ref * w.double()).sum().backward()
    close(kps.detach(), ref.detach(), "joints")
    close(xd.grad, x64.grad, "joint gradient")
    assert torch.all(xd.grad[:, J.shape[1]:] == 0)                          # the dummy row
    from semantichuman_amd import ops
    g = w.to(dev()).contiguous()
    assert torch.equal(ops.joint_regress_bwd(g, Jd, x.shape[1]), ops.joint_regress_bwd(g, Jd, x.shape[1]))


def test_input_errors_match_the_forward_entry_points():
    g = np.load(os.path.join(GOLD, "measure.npz"))
    fac, epi = rings_of(g)
    rings = measure.GirthRings(fac, epi, dev())
    v = meshes(g["verts"], 2, seed=1).to(dev())
    for bad in (v.double(), v.transpose(1, 2).contiguous().transpose(1, 2)):
        with pytest.raises(RuntimeError):
            measure.girths(bad, rings)
    k = torch.zeros((2, 35, 3), device=dev())
    for bad in (k.double(), k.transpose(0, 1).contiguous().transpose(0, 1)):
        with pytest.raises(RuntimeError):
            measure.bone_lengths(bad, measure.Bones(C.SKL_LIST[1:], dev()))
    with pytest.raises(RuntimeError):
        measure.joints(v.double(), torch.zeros((35, 578), device=dev()))
