#!/usr/bin/env python3
"""What the rig form of the free-space / silhouette term costs.  The ellipsoid scene of tools/bench_depth.py at
640 x 480 seen by the V = 4 cameras of tools/bench_views.py's rig, the 6890-vertex semantic model of tools/bench_fit.py, batch
1 / 16 / 64, in one process, the legs alternated over --rounds, medians reported.
  * "term": value and gradient of scan.free_space(x, rig_field, pose=) - one camera launch, one forward, one backward - against
    the recipe it replaces: V one-view fields and V calls scan.free_space(x, field_v, pose=pose.compose(E_v)), summed; wall time
    between device synchronisations, `evals` calls each.
  * "kernels": the three new kernels per call, from the library's dispatch events, and the recipe's one-view kernels next to them.
  * "fit": a fit step (decode, objective, backward, Adam) against a 50 000-point scan without the term, with the rig term (the
    cameras computed once, as editing.fit_scan does) and with the recipe.
One JSON line, also written to --out.
    python tools/bench_free_space_views.py [--batches 1,16,64] [--rounds 3] [--out profiles/bench_free_space_views.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from semantichuman_amd import _lib, editing, scan                 # noqa: E402
from bench_depth import AXES, H, INTR, W, Z_CUT, scene            # noqa: E402
from bench_fit import build                                       # noqa: E402
from bench_scan import time_fit                                   # noqa: E402
from bench_surface import kernels_of                              # noqa: E402
from bench_views import V, rig                                    # noqa: E402

NEW = ("free_space_cameras_kernel", "free_space_views_fwd_kernel", "free_space_views_bwd_kernel")
OLD = ("free_space_fwd_kernel", "free_space_bwd_kernel")


def wall_per_call(fn, evals):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(evals):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / evals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--form", default="planes3")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, _, h = build(dev)
    m.set_compute_dtype(torch.float32)
    _lib.set_f32_mma_mode(a.form)
    n, M = h.sizes[0], a.points
    res = {"metric": "free_space_views_cost", "image": [H, W], "views": V, "model": "semantic 6890", "points": M, "steps": a.steps,
           "evals": a.evals, "rounds": a.rounds, "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0), "legs": {}}
    med = lambda v: round(float(np.median(v)), 4)
    for B in [int(b) for b in a.batches.split(",")]:
        centres = np.stack([scene(B, seed=10 * B + v)[1] for v in range(V)], 1)               # [B, V, 3], each in its camera's frame
        depth = torch.from_numpy(np.stack([scene(B, seed=10 * B + v)[0] for v in range(V)], 1)).to(dev).contiguous()
        ext = rig(B)
        # the rig's cameras look at its origin from 2.2 m; every image shows its ellipsoid near (0, 0, 2.2): in the rig's frame, near the origin
        field = scan.DepthField.from_depth(depth, INTR, dev, extrinsics=ext, z_range=(0.5, Z_CUT))
        fields = [scan.DepthField.from_depth(depth[:, v].contiguous(), INTR, dev, z_range=(0.5, Z_CUT)) for v in range(V)]
        gen = torch.Generator().manual_seed(B)
        z = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        z_kps = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        dummy = editing._default_dummy(m, z)
        with torch.no_grad():
            x = m.decode(z, z_kps, dummy).contiguous()
            x_t = m.decode(z * 1.1, z_kps, dummy)[:, :n]
            pick = torch.randint(0, n, (B, M), generator=gen).to(dev)
            scans = scan.ScanBatch(torch.gather(x_t, 1, pick[:, :, None].expand(-1, -1, 3)).contiguous(), dev)
            lo, hi = x[:, :n].amin(1), x[:, :n].amax(1)
            s = (hi - lo).amax(1) / (2 * AXES[1])                                            # model units per metre
            A = torch.eye(3, device=dev)[None] * s[:, None, None]
            t = (lo + hi) / 2                                                                # the rig's origin sits in the body's centre
        pose = scan.Pose(A, t, s)
        E = [scan.Pose(torch.from_numpy(ext[:, v, :, :3].copy()).to(dev), torch.from_numpy(ext[:, v, :, 3].copy()).to(dev), torch.ones(B))
             for v in range(V)]
        plain = lambda xh: scan.chamfer(xh, scans, None, None, None, 0.5)

        def rig_term(xh, cameras=None):
            free, sil = scan.free_space(xh, field, pose=pose, cameras=cameras)
            return free + sil

        def recipe_term(xh):
            total = 0
            for v in range(V):
                free, sil = scan.free_space(xh, fields[v], pose=pose.compose(E[v]))
                total = total + (free + sil)
            return total

        def value_and_gradient(term):
            xg = x.clone().requires_grad_(True)
            term(xg).sum().backward()
            return xg.grad

        g_rig, g_recipe = value_and_gradient(rig_term), value_and_gradient(recipe_term)
        with torch.no_grad():
            agree = float((g_rig - g_recipe).abs().max() / g_recipe.abs().max().clamp_min(1e-30))
            cam = scan.free_space_cameras(field, pose)
            kinds, counts = scan.free_space_kinds(x, field, pose=pose)
        w_rig, w_recipe, k_rig, k_recipe, fit, fit_rig, fit_recipe = [], [], [], [], [], [], []
        for _ in range(a.rounds):                                                            # alternated in one process
            w_rig.append(wall_per_call(lambda: value_and_gradient(rig_term), a.evals))
            w_recipe.append(wall_per_call(lambda: value_and_gradient(recipe_term), a.evals))
            k_rig.append(kernels_of(lambda: value_and_gradient(rig_term), evals=3))
            k_recipe.append(kernels_of(lambda: value_and_gradient(recipe_term), evals=3))
            fit.append(time_fit(m, z, z_kps, dummy, plain, a.steps)[0])
            fit_rig.append(time_fit(m, z, z_kps, dummy, lambda xh: plain(xh) + rig_term(xh, cam), a.steps)[0])
            fit_recipe.append(time_fit(m, z, z_kps, dummy, lambda xh: plain(xh) + recipe_term(xh), a.steps)[0])
        new = {k: med([r.get(k, 0.0) for r in k_rig]) for k in NEW}
        old = {k: med([r.get(k, 0.0) for r in k_recipe]) for k in OLD}                       # the sum of the V calls
        f0, f1, f2 = med(fit), med(fit_rig), med(fit_recipe)
        res["legs"]["B%d" % B] = {
            "term": {"rig_ms": med(w_rig), "recipe_ms": med(w_recipe), "recipe_over_rig": round(med(w_recipe) / med(w_rig), 3),
                     "gradient_max_difference_relative": agree},
            "kernels": {"rig_ms": new, "rig_total_ms": round(sum(new.values()), 4), "recipe_ms_sum_of_V_calls": old},
            "fit": {"fit_step_ms": f0, "with_rig_term_ms": f1, "with_recipe_ms": f2, "rig_step_ratio": round(f1 / f0, 4),
                    "recipe_step_ratio": round(f2 / f0, 4), "rig_term_share_per_camera": round((f1 - f0) / f0 / V, 5),
                    "rig_kernels_over_step": round((new[NEW[1]] + new[NEW[2]]) / f0, 5)},
            "counts_active_free_silhouette_outside_per_view": counts.sum(0).tolist(),
            "ellipsoid_centres_spread_m": round(float(np.abs(centres - centres.mean((0, 1))).max()), 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
