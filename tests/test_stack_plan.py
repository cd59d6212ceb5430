"""The kernel-form plan of the fp32 stack sequencers (sh_stack_plan_f32, csrc/stack_exec.hip): what the forward pass writes and
what the backward pass reads agree, and every form the plan picks is one the kernels take.  The plan reads the step tables' shapes,
never their contents, so those tests build the stacks and "upload" them to the CPU; two GPU tests run the planes3 training step
where the forward and backward plane forms of a layer differ, against the exact form."""
import os

import numpy as np
import pytest
import torch

import semantichuman_amd as sh
from semantichuman_amd import _lib
from semantichuman_amd.hierarchy import load_hierarchy
from semantichuman_amd.stack import ConvStep, Stack

F = _lib.FORM
FE = [[3, 16, 32, 64, 128], [[], [], [], [], []]]
FD = [[128, 64, 32, 32, 16], [[], [], [], [], 3]]
BATCHES = (16, 48, 64, 272, 512, 1024)


def _flags(v):
    return [n for n in F if v & F[n]]


def _model_stacks(tpl):
    h = load_hierarchy(os.path.join(os.path.dirname(__file__), "golden", tpl))
    m = sh.SpiralAutoencoder(FE, FD, 256, h.sizes, h.spiral_sizes, h.spirals, h.D, h.U, torch.device("cpu"))
    return [(m._enc_stack, 3, "bm", False), (m._dec_stack, 128, "bm", True)]


def _sweep_stacks():
    """Conv chains with 48, 96 and 160 channels and spiral lengths 8 ... 25 (none of them shipped)."""
    rng = np.random.default_rng(5)
    out = []
    for S in (8, 9, 12, 16, 25):
        for chans in ([16, 32, 96, 48, 32, 16, 3], [32, 160, 96, 32], [64, 96, 96, 32, 48, 16]):
            steps, n = [], 320
            for j, (ci, co) in enumerate(zip(chans[:-1], chans[1:])):
                table = rng.integers(0, n, size=(n, S)).astype(np.int32)
                table[:, 0] = np.arange(n)                              # every row a source of itself: no empty transposed list
                steps.append(ConvStep(param=j, table=table, n_in=n, cin=ci, cout=co, act=1))
            out.append((Stack(steps).to(torch.device("cpu")), chans[0], "vm", True))
    return out


def _consumer(stack, i):
    j = i + 1
    if j < len(stack.steps) and stack.steps[j].kind == "spmm" and stack.steps[j].extend:
        j += 1
    return j if j < len(stack.steps) and stack.steps[j].kind == "conv" else -1


def _check(stack, c0, layout, need_x_grad, B):
    lib = _lib.load()
    f = stack.forms(B, c0, "planes3", layout, 2, need_x_grad)
    steps = stack.steps
    for i, st in enumerate(steps):
        has = lambda name: bool(f[i] & F[name])                    # noqa: E731
        # the backward pass reads an input image only where the forward pass writes one
        if has("bwd_p3w") or has("bwd_yimg"):
            assert i > 0 and f[i - 1] & F["fwd_img"], (i, _flags(f[i]), _flags(f[i - 1]))
        # fp32 rows are dropped only where the backward pass reads nothing but the image
        if has("fwd_img_only"):
            c = _consumer(stack, i)
            assert c > 0 and f[c] & F["bwd_p3w"] and f[c] & F["bwd_in_img_only"], (i, c)
            assert steps[c - 1].kind != "conv" or f[c] & F["bwd_yimg"], (i, c)
        if has("bwd_in_img_only"):
            assert has("bwd_p3w") and (steps[i - 1].kind != "conv" or has("bwd_yimg")), i
        if has("bwd_grad_img_only"):
            assert has("bwd_p3w") and (has("bwd_rag") or has("bwd_grp") or st.tt.n1 + st.tt.n2 == 0), i
        # every form the plan picks is taken by the kernels
        if st.kind != "conv":
            assert not f[i] & ~(F["fwd_img"] | F["fwd_img_only"]), (i, _flags(f[i]))
            continue
        if has("fwd_p3"):
            assert lib.sh_spiral_conv_p3_ok(B, st.S, st.cin, st.cout) and not (st.cout <= 16 and B > 256)
        if has("fwd_grp"):
            assert has("fwd_p3") and lib.sh_spiral_conv_p3_grp_ok(B, st.S, st.cin, st.cout, int(st.fgrp[0].shape[1]))
        if has("bwd_p3"):
            assert has("bwd_gimg") and lib.sh_spiral_conv_p3_ok(B, st.S, st.cout, st.cin)
        if has("bwd_rag"):
            assert has("bwd_p3") and lib.sh_spiral_conv_p3_rag_ok(B, st.S, st.cout, st.cin, int(st.rag[0].shape[1]))
        if has("bwd_grp"):
            assert has("bwd_p3") and lib.sh_spiral_conv_p3_grp_ok(B, st.S, st.cout, st.cin, int(st.bgrp[0].shape[1]))
        if has("bwd_p3w"):
            assert has("bwd_p3") and lib.sh_spiral_conv_bwd_wgt_p3_ok(B, st.R, st.S, st.cin, st.cout)
        if has("bwd_thin"):
            assert not has("bwd_p3") and lib.sh_spiral_conv_bwd_wgt_thin_ok(B, st.n_in, st.S, st.cin, st.cout, 0)
    return f


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("tpl", ["template6890.npz", "template27554.npz"])
def test_plan_of_the_shipped_models(tpl, B):
    for stack, c0, layout, need_x_grad in _model_stacks(tpl):
        _check(stack, c0, layout, need_x_grad, B)


@pytest.mark.parametrize("B", BATCHES)
def test_plan_of_other_filters(B):
    for stack, c0, layout, need_x_grad in _sweep_stacks():
        _check(stack, c0, layout, need_x_grad, B)


def test_plan_of_the_headline_step():
    """The forms of the benchmark's training step (6890 vertices, B = 64, planes3, keep_fp32 == 2), step by step."""
    (enc, *ea), (dec, *da) = _model_stacks("template6890.npz")
    grp_p3w = ["bwd_gimg", "bwd_p3", "bwd_grp", "bwd_p3w"]
    want_enc = [["fwd_img"],
                ["fwd_p3", "fwd_img", "fwd_img_only"] + grp_p3w + ["bwd_yimg", "bwd_in_img_only", "bwd_grad_img_only"],
                ["fwd_p3", "fwd_img", "fwd_img_only", "bwd_gimg", "bwd_p3", "bwd_rag", "bwd_presum_img", "bwd_p3w", "bwd_yimg",
                 "bwd_in_img_only", "bwd_grad_img_only"],
                ["fwd_p3", "bwd_gimg", "bwd_p3", "bwd_ride", "bwd_presum_img", "bwd_p3w", "bwd_yimg", "bwd_in_img_only"]]
    want_dec = [["fwd_img", "fwd_img_only"],
                ["fwd_p3", "fwd_img", "bwd_gimg", "bwd_p3", "bwd_ride", "bwd_presum_img", "bwd_p3w", "bwd_in_img_only"],
                ["fwd_img", "fwd_img_only"],
                ["fwd_p3", "fwd_img"] + grp_p3w + ["bwd_in_img_only", "bwd_grad_img_only"],
                ["fwd_img", "fwd_img_only"],
                ["fwd_p3", "fwd_grp", "fwd_img"] + grp_p3w + ["bwd_in_img_only", "bwd_grad_img_only"],
                ["fwd_img"],
                ["fwd_p3", "fwd_grp", "bwd_gimg", "bwd_p3", "bwd_grp", "bwd_presum_img"],
                ["bwd_thin"]]
    assert [_flags(v) for v in _check(enc, *ea, 64)] == want_enc
    assert [_flags(v) for v in _check(dec, *da, 64)] == want_dec


def test_no_plane_form_without_planes3():
    (enc, *ea), (dec, *da) = _model_stacks("template6890.npz")
    for stack, c0, layout, nxg in ((enc, *ea), (dec, *da)):
        for mma in ("exact", "split3"):
            f = stack.forms(64, c0, mma, layout, 1, nxg)
            assert all(v & ~(F["bwd_thin"] | F["bwd_ride"]) == 0 for v in f), [_flags(v) for v in f]


def test_plane_predicates_refuse_unbuilt_tile_counts():
    """The 16-channel plane kernels are built for one or two channel tiles per workgroup (csrc/p3_conv.hip p3_nt_built)."""
    lib = _lib.load()
    for S in (4, 8, 9, 12, 25):
        for n in range(4, 257, 4):
            if lib.sh_spiral_conv_p3_ok(64, S, 16, n):
                assert n <= 32 and lib.sh_spiral_conv_p3_kind(64, S, 16, n) == 1, (S, n)
    assert lib.sh_spiral_conv_p3_ok(64, 9, 16, 32) and not lib.sh_spiral_conv_p3_ok(64, 9, 16, 64)


# one training step (forward, L1 + 1e-2 x edge-ratio loss, backward) in a child process: argv = template, batch, FE, FD, latent size,
# form, output file; the arenas are poisoned with NaN (SH_DEBUG_POISON=1), so a read of a row no pass wrote would surface
_STEP = r"""
import json, sys
import numpy as np, torch
import semantichuman_amd as sh
from semantichuman_amd import _lib, synthetic
from semantichuman_amd.hierarchy import load_hierarchy
tpl, B, fe, fd, nz, form, out = sys.argv[1], int(sys.argv[2]), json.loads(sys.argv[3]), json.loads(sys.argv[4]), int(sys.argv[5]), sys.argv[6], sys.argv[7]
dev = torch.device("cuda:0")
h = load_hierarchy(tpl)
_lib.set_f32_mma_mode(form)
torch.manual_seed(11)
m = sh.SpiralAutoencoder(fe, fd, nz, h.sizes, h.spiral_sizes, h.spirals, h.D, h.U, dev)
x = torch.from_numpy(synthetic.synth_batch(h.verts, B, seed=4)).to(dev)
ft = sh.FaceTables(h.faces, h.sizes[0] + 1, dev)
n0 = _lib.load().sh_p3_launch_count()
x_hat, z = m(x)
loss = sh.l1_loss(x, x_hat) + 1e-2 * sh.edge_ratio_loss(x_hat, x, ft)
loss.backward()
torch.cuda.synchronize()
res = {"loss": loss.detach().cpu().numpy(), "x_hat": x_hat.detach().cpu().numpy(), "p3_launches": np.int64(_lib.load().sh_p3_launch_count() - n0)}
res.update({"grad." + n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()})
np.savez(out, **res)
"""


def _step(tmp_path, tpl, B, fe, fd, nz, form):
    import json
    import subprocess
    import sys
    out = str(tmp_path / ("%s_%s_%d.npz" % (form, tpl.split(".")[0], B)))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _STEP, os.path.join(root, "tests", "golden", tpl), str(B), json.dumps(fe), json.dumps(fd), str(nz),
                        form, out], env=dict(os.environ, SH_DEBUG_POISON="1"), capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return dict(np.load(out))


def _planes3_matches_exact(tmp_path, tpl, B, fe, fd, nz):
    """test_headline's tolerances: forward 1e-5, gradients 1e-4 of the largest magnitude."""
    ref, got = _step(tmp_path, tpl, B, fe, fd, nz, "exact"), _step(tmp_path, tpl, B, fe, fd, nz, "planes3")
    assert got["p3_launches"] > 0 and ref["p3_launches"] == 0
    for k in ref:
        if k == "p3_launches":
            continue
        tol = 1e-4 if k.startswith("grad.") else 1e-5
        assert np.isfinite(got[k]).all(), k
        err, scale = np.abs(got[k] - ref[k]).max(), np.abs(ref[k]).max()
        assert err <= tol * scale + 1e-30, "%s: err %.3e > %.1e * %.3e" % (k, err, tol, scale)


@pytest.mark.gpu
def test_planes3_step_with_other_filters_matches_exact(tmp_path):
    """A 32 -> 96 layer (S = 8) whose backward pass takes the plane kernels and whose forward pass does not: the image of its input
    is never written, and neither its weight gradient nor its activation derivative may read it."""
    _planes3_matches_exact(tmp_path, "small_ae.npz", 32, [[3, 16, 32, 96, 48], [[], [], [], [], []]],
                           [[48, 96, 32, 32, 16], [[], [], [], [], 3]], 16)


@pytest.mark.gpu
def test_planes3_step_at_batch_512_matches_exact(tmp_path):
    """The shipped filters at a batch where the 16-output-channel layer leaves the plane forward kernel (SH_P3_N16_MAXB)."""
    _planes3_matches_exact(tmp_path, "template6890.npz", 512, FE, FD, 256)
