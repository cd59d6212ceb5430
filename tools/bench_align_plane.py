#!/usr/bin/env python3
"""Time the point-to-plane pose step on the 6890-vertex semantic model (built as tools/bench_fit.py builds it) against M-point
Morton-sorted scans sampled on each body's own surface and moved by a similarity, batch 1 / 16 / 64, scan -> model only ("one")
and both directions ("both"); same process, alternated, kernel times from the library's dispatch events:
  * align_plane_moments_kernel (vertex and surface form) and align_plane_solve_kernel against align_moments_kernel /
    align_moments_surface_kernel and align_solve_kernel, per launch, and the search kernels of the same iteration;
  * the backward kernel of one register_scan step's surface Chamfer loss (surface_bwd_kernel), which the two new kernels are
    expected to stay under together;
  * one scan.align(faces=, step="plane") iteration against one step="point" iteration;
  * the iteration at which each loop first brings every body of the batch below 1e-3 of the extent (pose error: the largest
    displacement of a scan point from its true place), and the error after --iters iterations.
One JSON line, also written to --out.
    python tools/bench_align_plane.py [--batches 1,16,64] [--points 50000] [--steps 10] [--rounds 3] [--out profiles/bench_align_plane.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from semantichuman_amd import _lib, editing, scan                # noqa: E402
from bench_fit import build                                       # noqa: E402
from bench_align import timed                                     # noqa: E402
from bench_align_surface import sample_surface                    # noqa: E402

KERNELS = ("align_moments_kernel", "align_moments_surface_kernel", "align_solve_kernel", "align_plane_moments_kernel",
           "align_plane_moments_surface_kernel", "align_plane_solve_kernel", "transform_points_kernel", "vertex_normals_kernel",
           "nearest_search_kernel", "surface_search_kernel", "surface_bwd_kernel")


def kernel_ms(fn):
    _lib.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    rec = _lib.profile_records_by_kernel()
    _lib.profile_enable(False)
    out = {}
    for k in KERNELS:
        ms = [t for name, _, t in rec if name == k]
        if ms:
            out[k] = round(sum(ms) / len(ms), 5)
    return out


def first_below(x0, moved, truth_points, extent, ft, step, iters, level=1e-3):
    """(first iteration after which every body's pose error lies below `level` of its extent, or None; the error after `iters`).
    One align call per iteration count would repeat the work, so the loop is run once per count only up to the first hit."""
    err = None
    for k in range(1, iters + 1):
        _, al, _ = scan.align(x0, moved, mode="similarity", iters=k, w_model_to_scan=0.0, faces=ft, step=step)
        err = float(((al.points - truth_points).norm(dim=2).amax(1) / extent).max())
        if err < level:
            _, al, _ = scan.align(x0, moved, mode="similarity", iters=iters, w_model_to_scan=0.0, faces=ft, step=step)
            return k, float(((al.points - truth_points).norm(dim=2).amax(1) / extent).max())
    return None, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--form", default="planes3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, _, h = build(dev)
    m.set_compute_dtype(torch.float32)
    _lib.set_f32_mma_mode(a.form)
    n, M = h.sizes[0], a.points
    faces = np.asarray(h.faces, np.int64)
    ft = scan.FaceTable(faces, n, dev)
    res = {"metric": "align_plane_iteration_ms", "model": "semantic 6890", "faces": int(faces.shape[0]), "points": M, "form": a.form,
           "steps": a.steps, "rounds": a.rounds, "iters": a.iters, "build_id": _lib.build_id(), "legs": {}}
    th = np.deg2rad(10.0)
    Rz = torch.tensor([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    for B in [int(s) for s in a.batches.split(",")]:
        gen = torch.Generator().manual_seed(B)
        z = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        z_kps = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        dummy = editing._default_dummy(m, z)
        with torch.no_grad():
            x0 = m.decode(z, z_kps, dummy)
            own = sample_surface(x0[:, :n], faces, M, gen)
        away = scan.Pose((0.9 * Rz)[None].expand(B, -1, -1).contiguous(), torch.tensor([[0.05, -0.03, 0.04]]).expand(B, -1).contiguous())
        away = scan.Pose.from_packed(away.packed.to(dev), away.scale.to(dev))
        own_sb = scan.ScanBatch(own.cpu().numpy(), dev, order="morton")
        moved = away.apply(own_sb)
        extent = (x0[:, :n].amax(1) - x0[:, :n].amin(1)).amax(1)
        del own
        conv = {}
        for step in ("point", "plane"):
            k, err = first_below(x0, moved, own_sb.points, extent, ft, step, a.iters)
            conv[step] = {"first_iteration_below_1e-3": k, "pose_error_over_extent_after_%d" % a.iters: err}
        for leg, w in (("one", 0.0), ("both", 0.5)):
            def icp(step, iters, f=ft):
                return lambda: scan.align(x0, moved, iters=iters, w_model_to_scan=w, faces=f, step=step, **({} if f is not None else
                                                                                                             {"normal_faces": ft}))

            def reg(step, steps):
                return lambda: editing.register_scan(m, z, z_kps, moved, steps=steps, lr=1e-3, w_model_to_scan=w, align_iters=0, align_every=1,
                                                     dummy=dummy, faces=ft, align_on="surface", align_step=step)
            icp("point", 2)(); icp("plane", 2)(); reg("plane", 2)()                           # warm-up (allocator, plans, code objects)
            t = {"point": [], "plane": []}
            for _ in range(a.rounds):                                                         # alternated in one process
                for step in ("point", "plane"):
                    t[step].append(timed(icp(step, a.steps), a.steps)[0])
            km = kernel_ms(icp("point", 3))
            km.update({k: v for k, v in kernel_ms(icp("plane", 3)).items() if k.startswith(("align_plane", "vertex_normals"))})
            km.update({k: v for k, v in kernel_ms(icp("point", 3, None)).items() if k == "align_moments_kernel"})
            km.update({k: v for k, v in kernel_ms(icp("plane", 3, None)).items() if k == "align_plane_moments_kernel"})
            km.update({k: v for k, v in kernel_ms(reg("plane", 3)).items() if k == "surface_bwd_kernel"})
            res["legs"]["B%d_%s" % (B, leg)] = {
                "align_iteration_ms": {s: round(float(np.median(t[s])), 4) for s in t}, "kernel_ms_per_launch": km,
                "recovery_scan_to_model_only": conv}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
