"""Girth-targeted editing (editing.fit_latents / fit_part_girths) on the semantic.npz model with the golden girth rings.
Targets are reachable: z* = encode(x), target = girths(decode(z*)); the fit starts from z* with the edited parts scaled
by 1.3 (demo.py's size edit) and must find the girths again."""
import os

import numpy as np
import pytest
import torch

import semantichuman_amd as sh
from semantichuman_amd import _lib
from semantichuman_amd import constants as C
from semantichuman_amd import editing, measure
from semantichuman_amd.hierarchy import load_hierarchy

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SCALED = [2, 3, 4]                                   # parts whose size the start edits (demo.py's 1.3)
PARTS = list(range(1, 16))                           # the latents the fits move (parts 0 and 16 stay: they must come back bitwise)
EDIT, HOLD = [0, 1, 2, 3], [4, 5, 6, 7]


def semantic_setup(B=3, seed=0, dtype=torch.float32, scaled=SCALED):
    dev = torch.device("cuda:0")
    gs = np.load(os.path.join(GOLD, "semantic.npz"))
    gm = np.load(os.path.join(GOLD, "measure.npz"))
    h = load_hierarchy(os.path.join(GOLD, "semantic.npz"))
    coarse = {n: gs["part_coarse_%d" % k] for k, n in enumerate(C.PART_LIST)}
    m = sh.SpiralAutoencoder_multiz_partkps(C.KPS_INDEX_LIST, coarse, C.FILTER_SIZES_ENC, C.FILTER_SIZES_DEC, 8, 8, h.sizes,
                                            h.spiral_sizes, h.spirals, h.D, h.U, dev)
    m.load_state_dict({k[3:]: torch.from_numpy(gs[k]) for k in gs.files if k.startswith("w0/")})
    m.set_compute_dtype(dtype)                                  # targets decoded in the fit's own arithmetic: reachable
    n = int(gm["n_planes"])
    rings = measure.GirthRings([gm["factor_%d" % i] for i in range(n)], [gm["epi_%d" % i] for i in range(n)], dev)
    idx = torch.arange(B) % 3
    gen = torch.Generator().manual_seed(seed)
    x = torch.from_numpy(gs["x"])[idx]
    if B > 3:                                                   # different bodies (and so different targets) per batch entry
        x = x * (1 + 0.05 * torch.randn((B, 1, 3), generator=gen))
    x = x.to(dev).contiguous()
    kps = torch.from_numpy(gs["kps"])[idx].to(dev).contiguous()
    with torch.no_grad():
        z_star, z_kps, dummy = m.encode(x, kps)
        target = measure.girths(m.decode(z_star, z_kps, dummy), rings)[:, EDIT]
    z0 = editing.edit_part_size(z_star, scaled, 1.3)
    J = torch.from_numpy(gs["J_regressor"].astype(np.float32)).to(dev)
    return m, rings, z0, z_kps, dummy, target, J


def snapshot(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fit_part_girths_reaches_reachable_targets(dtype):
    # bf16: activations are rounded to 8 bits, so every decoded measurement carries ~1e-2 relative quantisation once the latents
    # move; a held girth or length (exact at the start by construction) then settles at that level (~3e-3 of loss over 24 terms).
    # The bf16 case therefore asks for a +5 % edit of the edited rings with nothing held - far above that floor.
    bf = dtype == "bf16"
    m, rings, z0, z_kps, dummy, target, J = semantic_setup(dtype=torch.bfloat16 if bf else torch.float32)
    with torch.no_grad():
        g_start = measure.girths(m.decode(z0, z_kps, dummy), rings)
    if bf:
        target = g_start[:, EDIT] * 1.05
    before = snapshot(m)
    name0 = next(iter(before))
    sentinel = torch.full_like(before[name0], 7.0)
    dict(m.named_parameters())[name0].grad = sentinel
    list(m.parameters())[1].requires_grad_(False)                     # a flag that is not the default comes back as it was
    flags = {n: p.requires_grad for n, p in m.named_parameters()}
    z_in, zk_in = z0.clone(), z_kps.clone()
    z1, g1, losses = editing.fit_part_girths(m, z0, z_kps, rings, target, EDIT, () if bf else HOLD, parts=PARTS, bones=C.SKL_LIST[1:],
                                             J=J, hold_lengths=not bf, steps=800, lr=2e-3, dummy=dummy)
    assert losses.is_cuda and losses.shape == (800,)
    l = losses.cpu()
    assert torch.isfinite(l).all()
    rel = ((g1[:, EDIT] - target) / target).abs().max().item()
    rel_hold = ((g1[:, HOLD] - g_start[:, HOLD]) / g_start[:, HOLD]).abs().max().item()
    if dtype == "fp32":
        assert (rel <= 1e-3 and rel_hold <= 1e-3) or float(l[-1]) <= float(l[0]) / 100, (rel, rel_hold, float(l[0]), float(l[-1]))
    else:
        assert float(l[-10:].min()) <= float(l[0]) / 100 and rel <= 1e-2, (rel, float(l[0]), float(l[-1]))
    # only z[:, PARTS] moved; z_kps, the inputs and all parameters are bitwise unchanged; flags and .grad as they were
    others = [k for k in range(z0.shape[1]) if k not in PARTS]
    assert torch.equal(z1[:, others], z0[:, others]) and not torch.equal(z1[:, PARTS], z0[:, PARTS])
    assert torch.equal(z0, z_in) and torch.equal(z_kps, zk_in)
    for n, p in m.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
        assert p.requires_grad == flags[n], n
    assert dict(m.named_parameters())[name0].grad is sentinel and torch.all(sentinel == 7.0)
    assert all(p.grad is None for n, p in m.named_parameters() if n != name0)


def test_fit_is_deterministic_and_skips_weight_gradients():
    m, rings, z0, z_kps, dummy, target, _ = semantic_setup()
    _lib.profile_enable(True)
    a = editing.fit_part_girths(m, z0, z_kps, rings, target, EDIT, HOLD, parts=PARTS, steps=40, lr=1e-2, dummy=dummy)
    torch.cuda.synchronize()
    names = {n for n, _, _ in _lib.profile_records_by_kernel()}
    _lib.profile_enable(False)
    b = editing.fit_part_girths(m, z0, z_kps, rings, target, EDIT, HOLD, parts=PARTS, steps=40, lr=1e-2, dummy=dummy)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert "girth_bwd_kernel" in names
    assert not [n for n in names if n.startswith("wgrad") or "bwd_wgt" in n or "slab_reduce" in n], sorted(names)


def test_batched_fit_matches_single_body_fits():
    B = 16
    m, rings, z0, z_kps, dummy, target, _ = semantic_setup(B=B, seed=4)
    assert float((target[0] - target[3]).abs().max()) > 0                  # the bodies really have different targets
    zb, gb, _ = editing.fit_part_girths(m, z0, z_kps, rings, target, EDIT, HOLD, parts=PARTS, steps=60, lr=1e-2, dummy=dummy)
    for b in (0, 5, 11):
        s = slice(b, b + 1)
        z1, g1, _ = editing.fit_part_girths(m, z0[s], z_kps[s], rings, target[s], EDIT, HOLD, parts=PARTS, steps=60, lr=1e-2,
                                            dummy=dummy[s])
        assert float((z1 - zb[s]).abs().max()) <= 1e-5 * float(zb[s].abs().max()), b
        assert float(((g1 - gb[s]) / gb[s]).abs().max()) <= 1e-5, b


@pytest.mark.parametrize("f32_mma", ["planes3"], indirect=True)
def test_fit_latents_inversion_at_size(f32_mma):
    """One L1 inversion through the 6890-vertex plain autoencoder at batch 64 in the three-plane form."""
    from semantichuman_amd import synthetic
    dev = torch.device("cuda:0")
    h = load_hierarchy(os.path.join(GOLD, "template6890.npz"))
    torch.manual_seed(5)
    m = sh.SpiralAutoencoder([[3, 16, 32, 64, 128], [[], [], [], [], []]], [[128, 64, 32, 32, 16], [[], [], [], [], 3]], 256, h.sizes,
                             h.spiral_sizes, h.spirals, h.D, h.U, dev)
    x = torch.from_numpy(synthetic.synth_batch(h.verts, 64, seed=3)).to(dev)
    with torch.no_grad():
        z_star = m.encode(x)
        x_star = m.decode(z_star)
    before = snapshot(m)
    z0 = z_star * 1.3
    z1, losses = editing.fit_latents(m, z0, None, lambda xh: (xh - x_star).abs().mean((1, 2)), None, steps=40, lr=1e-2)
    l = losses.cpu()
    assert torch.isfinite(l).all() and float(l[-1]) < 0.5 * float(l[0]), (float(l[0]), float(l[-1]))
    assert z1.shape == z0.shape and not torch.equal(z1, z0)
    for n, p in m.named_parameters():
        assert torch.equal(p.detach(), before[n]) and p.requires_grad and p.grad is None, n
