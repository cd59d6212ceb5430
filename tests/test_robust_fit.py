"""The robust terms through editing.fit_scan and editing.register_scan: a short fit on semantic.npz against scans with one-sided
outliers ends nearer the true body with robust="geman-mcclure" than without it - and so does the same fit under the plain-torch
objective of tests/test_scan.py, the yardstick that shows the ordering belongs to the inputs and not to the kernels -; every
place the two functions hand the robust term on (stage-1 align, the fit's forward and backward pass with and without
visibility, the in-loop pose update, the final value) launches the robust kernels and no plain one; and robust=None launches
what the call without the argument launches, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from semantichuman_amd import editing, scan
from tests.launch_record import launches
from tests.test_align_surface import same
from tests.test_scan import PARTS, semantic_setup
from tests.test_surface_gated import fit_setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTLIER_SHARE, OUTLIER_SIGMA, STEPS, LR = 0.15, 0.03, 300, 5e-3
# the kernels that carry the penalty or the weight, by their plain names; the robust forms insert "_robust" before "_kernel"
PLAIN = {"chamfer_fwd_kernel", "chamfer_bwd_kernel", "surface_bwd_kernel", "align_moments_kernel", "align_moments_surface_kernel",
         "align_plane_moments_kernel", "align_plane_moments_surface_kernel"}


def robust_name(k):
    return k.replace("_kernel", "_robust_kernel")


@functools.lru_cache(maxsize=None)
def outlier_fit_inputs():
    """test_scan.semantic_setup's model, start and scans (the true body's vertices, permuted), each scan with 15 % extra points
    drawn uniformly in a box of 0.3 of the extent that hangs on the +x side of the body - a hand-held object; sigma = 0.03 of the
    extent."""
    m, z0, z_kps, dummy, scans, x_star, n = semantic_setup()
    xs = x_star[:, :n].cpu().numpy().astype(np.float64)
    pts = scans.points.cpu().numpy()
    clouds, extent = [], float((xs[0].max(0) - xs[0].min(0)).max())
    for b in range(xs.shape[0]):
        rs = np.random.RandomState(31 + b)
        lo = np.array([xs[b, :, 0].max() + 0.03 * extent, xs[b, :, 1].mean() - 0.15 * extent, xs[b, :, 2].mean() - 0.15 * extent])
        box = lo + rs.rand(int(round(OUTLIER_SHARE * n)), 3) * 0.3 * extent
        clouds.append(np.concatenate([pts[b, :n], box.astype(np.float32)]))
    return m, z0, z_kps, dummy, scan.ScanBatch(clouds, DEV), x_star, n, OUTLIER_SIGMA * extent


def torch_chamfer(scans, n, scale2=None):
    """test_scan.torch_chamfer, and with scale2 its Geman-McClure form: the scan -> model objective a user could write in torch."""
    def objective(x_hat):
        d = (scans.points[:, :, None, :] - x_hat[:, None, :n, :]).pow(2).sum(-1).min(2).values
        return (d if scale2 is None else d * scale2 / (scale2 + d)).mean(1)
    return objective


def test_fit_scan_with_outliers_ends_nearer_the_true_body():
    m, z0, z_kps, dummy, sb, x_star, n, sigma = outlier_fit_inputs()

    def distance(z):
        with torch.no_grad():
            return (m.decode(z, z_kps, dummy)[:, :n] - x_star[:, :n]).norm(dim=2).mean().item()

    kw = dict(parts=PARTS, steps=STEPS, lr=LR, dummy=dummy)
    z_plain, _, _ = editing.fit_scan(m, z0, z_kps, sb, **kw)
    z_rob, final, losses = editing.fit_scan(m, z0, z_kps, sb, robust="geman-mcclure", robust_scale=sigma, **kw)
    zt_plain, _ = editing.fit_latents(m, z0, z_kps, torch_chamfer(sb, n), PARTS, steps=STEPS, lr=LR, dummy=dummy)
    zt_rob, _ = editing.fit_latents(m, z0, z_kps, torch_chamfer(sb, n, sigma * sigma), PARTS, steps=STEPS, lr=LR, dummy=dummy)
    d0, d_plain, d_rob, dt_plain, dt_rob = (distance(z) for z in (z0, z_plain, z_rob, zt_plain, zt_rob))
    print("fit_scan with outliers: mean vertex distance to x*: start %.4g, plain %.4g, geman-mcclure %.4g; torch objective: plain %.4g, "
          "geman-mcclure %.4g" % (d0, d_plain, d_rob, dt_plain, dt_rob))
    assert torch.isfinite(losses).all() and torch.isfinite(final).all()
    assert dt_rob < dt_plain, (dt_rob, dt_plain)                           # the ordering is the inputs': the torch objective shows it too
    assert d_rob < d_plain, (d_rob, d_plain)
    assert d_rob <= 1.10 * dt_rob, (d_rob, dt_rob)                         # test_scan's margin of the library's fit over the torch objective


@functools.lru_cache(maxsize=None)
def editing_inputs():
    m, z0, z_kps, dummy, x_star, n, faces, clouds, normals, trunc = fit_setup()
    keep = [300 - 11 * b for b in range(len(clouds))]
    view = np.tile(np.array([0.0, 0.0, 5.0], np.float32), (len(clouds), 1))                 # one sensor position per body, [B, 3]
    sb = scan.ScanBatch([c[:k] for c, k in zip(clouds, keep)], DEV, viewpoints=view)
    sigma = 0.05 * float(x_star[:, :n].abs().max())
    return m, z0, z_kps, dummy, faces, sb, trunc, sigma


def fit_run(**kw):
    m, z0, z_kps, dummy, faces, sb, trunc, sigma = editing_inputs()
    return list(editing.fit_scan(m, z0, z_kps, sb, parts=PARTS, steps=2, lr=1e-2, w_model_to_scan=0.5, trunc=trunc, dummy=dummy, **kw))


def register_run(**kw):
    m, z0, z_kps, dummy, faces, sb, trunc, sigma = editing_inputs()
    z, pose, final, losses = editing.register_scan(m, z0, z_kps, sb, parts=PARTS, mode="rigid", init="identity", align_iters=2, align_every=1,
                                                   steps=2, lr=1e-2, w_model_to_scan=0.5, trunc=trunc, dummy=dummy, **kw)
    return [z, pose.packed, pose.scale, final, losses]


def editing_cases():
    faces = editing_inputs()[4]
    vis = dict(visibility="viewpoint", visibility_faces=faces)
    return [(fit_run, {}), (fit_run, dict(faces=faces)), (fit_run, vis), (register_run, {}), (register_run, vis),
            (register_run, dict(faces=faces, align_on="surface")), (register_run, dict(faces=faces, align_on="surface", align_step="plane", **vis)),
            (register_run, dict(normal_faces=faces, align_step="plane"))]


def test_every_stage_of_the_editing_functions_runs_the_robust_kernels():
    """With a robust form, every kernel of PLAIN that the plain call launches is launched in its robust form instead - same
    order, same count - and no plain one is left: a stage that dropped the argument would launch one."""
    sigma = editing_inputs()[7]
    seen = set()
    for fn, base in editing_cases():
        ref, rec_ref = launches(lambda: fn(**base))
        on, rec_on = launches(lambda: fn(robust="geman-mcclure", robust_scale=sigma, **base))
        want = [robust_name(k) if k in PLAIN else k for k, _ in rec_ref]
        assert [k for k, _ in rec_on] == want, (fn.__name__, sorted(base))
        assert not {k for k, _ in rec_on} & PLAIN and not all(same(u, v) for u, v in zip(ref, on))
        seen |= {k for k, _ in rec_on if "robust" in k}
    assert seen == {robust_name(k) for k in PLAIN}, seen
    # register_scan, vertex pairs: stage 1 (two iterations: value, moments), two fit steps (value, gradient, then the pose
    # update's moments) and the final value - in that order
    _, rec = launches(lambda: register_run(robust="huber", robust_scale=sigma))
    names = [k for k, _ in rec if "robust" in k]
    fwd, bwd, mom = "chamfer_fwd_robust_kernel", "chamfer_bwd_robust_kernel", "align_moments_robust_kernel"
    assert names == [fwd, mom, fwd, mom, fwd, bwd, mom, fwd, bwd, mom, fwd], names


def test_robust_none_is_the_default_path_of_the_editing_functions():
    for fn, base in editing_cases():
        ref, rec_ref = launches(lambda: fn(**base))
        off, rec_off = launches(lambda: fn(robust=None, robust_scale=None, **base))
        assert rec_off == rec_ref and all(same(u, v) for u, v in zip(ref, off)), (fn.__name__, sorted(base))
        assert not any("robust" in k for k, _ in rec_off)
