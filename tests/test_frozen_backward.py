"""Backward passes of the conv stacks with frozen weights: a layer whose weight and bias are both frozen gets a NULL dW
(include/sh_kernels.h, sh_stack_backward) and launches no weight-gradient kernel; every gradient that is still computed is
the full backward's.

One stated exception.  The role-swapped 16 -> 3 weight-gradient kernel (wgrad_thin_kernel<...>, csrc/wgrad_thin.hip; batches
that are multiples of 16) also writes its layer's input gradient, in its own summation order.  When that layer is frozen, the
ordinary backward-data kernel of the step writes it instead - the kernel the full backward itself uses with SH_WGRAD_THIN=0.
So:
  * with the thin kernel switched off, the frozen and the full backward are bitwise equal (test_frozen_is_bitwise_without_
    the_thin_kernel, in a child process, at the headline size, in exact / planes3 / bf16);
  * with it on, gradients upstream of the frozen thin layer match the full backward within TOL (input / latent gradient) and
    PTOL (parameter gradients; the largest gap is a bias gradient, a sum over 64 x 3445 rows with cancellation), and they are
    no farther from the float64 oracle than the full backward's own (test_frozen_backward_vs_float64_oracle_at_size).
Everything else is compared bitwise."""
import os

import numpy as np
import pytest
import torch

import semantichuman_amd as sh
from semantichuman_amd import _lib
from semantichuman_amd import constants as C
from semantichuman_amd import editing
from semantichuman_amd.hierarchy import load_hierarchy

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FE_H = [[3, 16, 32, 64, 128], [[], [], [], [], []]]
FD_H = [[128, 64, 32, 32, 16], [[], [], [], [], 3]]
TOL = {"fp32": 1e-5, "bf16": 3e-2}         # input gradient, x max|g| (measured: 1.0e-6 exact, 7.5e-7 planes3, 2.8e-3 bf16)
PTOL = {"fp32": 3e-3, "bf16": 3e-2}        # parameter gradients (measured: 1.1e-3 on dconv.3's bias in exact and planes3, 1.2e-2 bf16)

# (model, batch, compute dtype, fp32 form); the form is applied by conftest through the f32_mma fixture; planes3 at B % 16 == 0
CASES = [("small", 3, "fp32", "exact"), ("small", 3, "fp32", "split3"), ("small", 3, "bf16", "exact"),
         ("semantic", 3, "fp32", "exact"), ("semantic", 3, "fp32", "split3"), ("semantic", 3, "bf16", "exact"),
         ("semantic", 16, "fp32", "planes3"), ("semantic", 16, "bf16", "exact"),
         ("headline", 64, "fp32", "exact"), ("headline", 64, "fp32", "split3"), ("headline", 64, "fp32", "planes3"),
         ("headline", 64, "bf16", "exact")]
ids = lambda cases: ["%s-B%d-%s" % (m, b, d if d == "bf16" else f) for m, b, d, f in cases]   # noqa: E731


def is_wgrad(name):
    return name.startswith("wgrad") or "bwd_wgt" in name or "slab_reduce" in name


def thin_ran(records):
    """Did the full backward run the role-swapped 16 -> 3 kernel (which writes its layer's input gradient)?"""
    return any(n.startswith("wgrad_thin_kernel") for n, _ in records)


def build(kind, B):
    dev = torch.device("cuda:0")
    if kind == "small":
        g = np.load(os.path.join(GOLD, "small_ae.npz"))
        h = load_hierarchy(os.path.join(GOLD, "small_ae.npz"))
        m = sh.SpiralAutoencoder([[3, 16, 32, 64, 128], [[], [], [], [], []]], [[128, 64, 32, 32, 16], [[], [], [], [], 3]], 16, h.sizes,
                                 h.spiral_sizes, h.spirals, h.D, h.U, dev)
        m.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w0/")})
        x = torch.from_numpy(g["x"])
        x = x[torch.arange(B) % x.shape[0]].contiguous()
        return m, (x.to(dev),)
    if kind == "headline":
        from semantichuman_amd import synthetic
        h = load_hierarchy(os.path.join(GOLD, "template6890.npz"))
        torch.manual_seed(20 + B)
        m = sh.SpiralAutoencoder(FE_H, FD_H, 256, h.sizes, h.spiral_sizes, h.spirals, h.D, h.U, dev)
        x = torch.from_numpy(synthetic.synth_batch(h.verts, B, seed=7)).to(dev)
        return m, (x,)
    gs = np.load(os.path.join(GOLD, "semantic.npz"))
    h = load_hierarchy(os.path.join(GOLD, "semantic.npz"))
    coarse = {n: gs["part_coarse_%d" % k] for k, n in enumerate(C.PART_LIST)}
    m = sh.SpiralAutoencoder_multiz_partkps(C.KPS_INDEX_LIST, coarse, C.FILTER_SIZES_ENC, C.FILTER_SIZES_DEC, 8, 8, h.sizes,
                                            h.spiral_sizes, h.spirals, h.D, h.U, dev)
    m.load_state_dict({k[3:]: torch.from_numpy(gs[k]) for k in gs.files if k.startswith("w0/")})
    gen = torch.Generator().manual_seed(B)
    idx = torch.arange(B) % 3
    z = torch.from_numpy(gs["z"])[idx] * (1 + 0.1 * torch.randn((B, 17, 1), generator=gen))
    zk = torch.from_numpy(gs["z_part_kps"])[idx]
    return m, (z.to(dev).contiguous(), zk.to(dev).contiguous())


def run(m, inp, kind, trainable):
    """One forward + backward with parameter `n` trainable iff trainable(n); the gradient source is the model input (x for the
    autoencoder, the part latents for the semantic model's decoder).  -> (input gradient, {name: grad}, kernel names)."""
    for n, p in m.named_parameters():
        p.grad = None
        p.requires_grad_(trainable(n))
    a = inp[0].clone().requires_grad_(True)
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    if kind == "semantic":
        out = m.decode(a, inp[1], editing._default_dummy(m, a))
    else:
        out = m(a)[0]
    w = torch.linspace(-1, 1, out.numel(), device=out.device).view(out.shape)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    names = {(n, tag) for n, tag, _ in _lib.profile_records_by_kernel()}
    _lib.profile_enable(False)
    grads = {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}
    for p in m.parameters():
        p.requires_grad_(True)
    return a.grad.clone(), grads, names


def same(got, ref, exact, what, tol):
    if exact:
        assert torch.equal(got, ref), what + ": not bitwise the full backward's"
    else:
        err = float((got - ref).abs().max()) / float(ref.abs().max())
        assert err <= tol, what + ": %.2e x max|g| from the full backward's (tolerance %.1e)" % (err, tol)


@pytest.mark.parametrize("f32_mma,cfg", [(c[3], c) for c in CASES], ids=ids(CASES), indirect=["f32_mma"])
def test_all_frozen_backward_skips_weight_gradients(f32_mma, cfg):
    kind, B, dt, _ = cfg
    m, inp = build(kind, B)
    if dt == "bf16":
        m.set_compute_dtype(torch.bfloat16)
    g_full, _, k_full = run(m, inp, kind, lambda n: True)
    g_frz, grads, k_frz = run(m, inp, kind, lambda n: False)
    assert any(is_wgrad(k) for k, _ in k_full), "the full backward lists weight-gradient kernels"
    bad = sorted({k for k, _ in k_frz if is_wgrad(k)})
    assert not bad, "weight-gradient kernels in a frozen backward: %s" % bad
    assert all(g is None for g in grads.values())
    same(g_frz, g_full, not thin_ran(k_full), "input gradient", TOL[dt])
    assert torch.isfinite(g_frz).all() and float(g_frz.abs().max()) > 0


def _partial_sets(m, kind):
    convs = [n for n, _ in m.named_parameters() if ".conv." in n]
    enc = [n for n in convs if n.startswith("conv.")]
    dec = [n for n in convs if n.startswith("dconv.")]
    layers = sorted({n.rsplit(".", 1)[0] for n in convs})
    alt = {l for i, l in enumerate(layers) if i % 2 == 0}
    sets = {"encoder": set(enc), "decoder": set(dec), "alternate": {n for n in convs if n.rsplit(".", 1)[0] in alt}}
    if kind == "semantic":                              # decode only: the encoder's convs take no part
        sets.pop("encoder")
    return sets, dec


@pytest.mark.parametrize("f32_mma,cfg", [(c[3], c) for c in CASES], ids=ids(CASES), indirect=["f32_mma"])
def test_partially_frozen_gradients_are_the_full_backwards(f32_mma, cfg):
    kind, B, dt, _ = cfg
    m, inp = build(kind, B)
    if dt == "bf16":
        m.set_compute_dtype(torch.bfloat16)
    g_full, full, k_full = run(m, inp, kind, lambda n: True)
    thin = thin_ran(k_full)
    sets, dec = _partial_sets(m, kind)
    last_dec = max(dec, key=lambda n: int(n.split(".")[1])).rsplit(".", 1)[0]
    for label, frozen in sets.items():
        g, grads, k = run(m, inp, kind, lambda n: n not in frozen)
        # bitwise unless the frozen set holds the thin layer: then its input gradient comes from the ordinary kernel
        thin_frozen = any(f.startswith(last_dec + ".") for f in frozen)
        assert not (thin_frozen and thin_ran(k)), "%s: a frozen thin layer still ran the role-swapped kernel" % label
        exact = not (thin and thin_frozen)
        for n, gr in grads.items():
            if n in frozen:
                assert gr is None, "%s: frozen %s has a .grad" % (label, n)
            elif full[n] is not None and (kind != "semantic" or not n.startswith(("conv.", "fc_latent_enc", "kps_enc"))):
                assert gr is not None, "%s: %s has no .grad" % (label, n)
                same(gr, full[n], exact, "%s: %s" % (label, n), PTOL[dt])
        same(g, g_full, exact, "%s: input gradient" % label, TOL[dt])


# ------------------------------------------------------------------------------------------ the thin layer, settled
def _bitwise_probe(form):
    """Child-process body (SH_WGRAD_THIN=0 is read once per process): headline model, all-frozen and alternate-frozen backward
    against the full backward, bitwise.  Prints one JSON line."""
    import json
    if form == "bf16":
        _lib.set_f32_mma_mode("exact")
    else:
        _lib.set_f32_mma_mode(form)
    m, inp = build("headline", 64)
    if form == "bf16":
        m.set_compute_dtype(torch.bfloat16)
    g_full, full, k_full = run(m, inp, "headline", lambda n: True)
    g_frz, _, k_frz = run(m, inp, "headline", lambda n: False)
    sets, _ = _partial_sets(m, "headline")
    g_alt, alt, _ = run(m, inp, "headline", lambda n: n not in sets["alternate"])
    print(json.dumps({"thin_ran": thin_ran(k_full), "wgrad_in_frozen": any(is_wgrad(n) for n, _ in k_frz),
                      "frozen_equal": bool(torch.equal(g_frz, g_full)), "alternate_equal": bool(torch.equal(g_alt, g_full)) and
                      all(torch.equal(alt[n], full[n]) for n in alt if n not in sets["alternate"])}))


@pytest.mark.parametrize("form", ["exact", "planes3", "bf16"])
def test_frozen_is_bitwise_without_the_thin_kernel(form):
    """The only difference between the frozen and the full backward at the headline size is the thin kernel's own arithmetic:
    with it switched off (a fresh child process with SH_WGRAD_THIN=0), they are bitwise equal."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SH_WGRAD_THIN="0")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests import test_frozen_backward as t; "
                        "t._bitwise_probe(%r)" % (root, form)], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["thin_ran"] and not res["wgrad_in_frozen"], res
    assert res["frozen_equal"] and res["alternate_equal"], res


@pytest.mark.parametrize("f32_mma", ["exact", "planes3"], indirect=True)
def test_frozen_backward_vs_float64_oracle_at_size(f32_mma):
    """With the thin kernel on, the frozen path's gradients are no farther from float64 than the full backward's own."""
    from oracle import ref_cpu
    from semantichuman_amd import synthetic
    h = load_hierarchy(os.path.join(GOLD, "template6890.npz"))
    m, inp = build("headline", 64)
    S = [torch.from_numpy(sp.astype(np.int64))[None] for sp in h.spirals]
    _, D, U = h.dense_constants()
    om = ref_cpu.SpiralAEOracle(FE_H, FD_H, 256, h.sizes, h.spiral_sizes, S, [d.double() for d in D], [u.double() for u in U]).double()
    om.load_state_dict({k: v.detach().cpu().double() for k, v in m.state_dict().items()})
    sets, _ = _partial_sets(m, "headline")
    frozen = sets["alternate"]
    for n, p in om.named_parameters():
        p.requires_grad_(n not in frozen)
    xo = inp[0].cpu().double().requires_grad_(True)
    out = om(xo)[0]
    w = torch.linspace(-1, 1, out.numel(), dtype=torch.float64).view(out.shape)
    (out * w).sum().backward()
    ref_x, ref_p = xo.grad, {n: p.grad for n, p in om.named_parameters() if p.grad is not None}
    g_full, full, k_full = run(m, inp, "headline", lambda n: True)
    g_alt, alt, _ = run(m, inp, "headline", lambda n: n not in frozen)
    g_frz, _, _ = run(m, inp, "headline", lambda n: False)
    assert thin_ran(k_full)
    rel = lambda a, b: float((a.double().cpu() - b).abs().max()) / float(b.abs().max())      # noqa: E731
    e_full = rel(g_full, ref_x)
    assert rel(g_frz, ref_x) <= 2 * e_full + 1e-6 and rel(g_alt, ref_x) <= 2 * e_full + 1e-6, (rel(g_frz, ref_x), e_full)
    for n in ref_p:                                     # (1e-4: the suite's gradient tolerance against the oracle, tests/test_headline.py)
        assert rel(alt[n], ref_p[n]) <= 2 * rel(full[n], ref_p[n]) + 1e-4, (n, rel(alt[n], ref_p[n]), rel(full[n], ref_p[n]))


@pytest.mark.parametrize("f32_mma", ["exact"], indirect=True)
def test_python_sequencer_honours_the_frozen_mask(f32_mma, monkeypatch):
    """The opt-in Python sequencer (SH_OVERLAP_WGRAD: weight gradients on a side stream) skips frozen layers too."""
    from semantichuman_amd import stack
    monkeypatch.setattr(stack, "OVERLAP_WGRAD", True)
    for kind, B in (("small", 3), ("headline", 64)):
        m, inp = build(kind, B)
        g_full, full, _ = run(m, inp, kind, lambda n: True)
        g_frz, grads, k = run(m, inp, kind, lambda n: False)
        assert not [n for n, _ in k if is_wgrad(n)] and all(g is None for g in grads.values())
        assert torch.equal(g_frz, g_full)                   # (this sequencer takes no thin kernel with a side stream)
        sets, _ = _partial_sets(m, kind)
        for label, frozen in sets.items():
            g, gr, _ = run(m, inp, kind, lambda n: n not in frozen)
            assert torch.equal(g, g_full), label
            for n in gr:
                assert (gr[n] is None) if n in frozen else torch.equal(gr[n], full[n]), (label, n)
