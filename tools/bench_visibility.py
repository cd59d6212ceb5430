#!/usr/bin/env python3
"""What the visibility mask of a partial scan costs.  The 6890-vertex template, batch 1 / 16 / 64, one viewpoint per
body off the symmetry planes, in one process, legs alternated, kernel times from the library's dispatch events, medians over the
rounds:
  * one visibility pass (vertex_visibility_kernel + visibility_fold_kernel) over synthetic.synth_batch bodies of the template -
    body-shaped, about a third of the vertices visible - plain and with grazing_angle (which adds vertex_normals_kernel);
  * one ungated sh_nearest_points(scan -> x) over M-point scans of the same bodies - the yardstick: the same brute-force form,
    6890 x M pairs against the pass's 6890 x 13776;
  * the same pass over what the semantic model of tools/bench_fit.py decodes (random weights: a crumpled surface on which
    nearly every vertex is hidden within a few tiles - the early exit's best case), and one fit step of that model (decode ->
    chamfer, both directions -> backward -> Adam) with and without visibility="viewpoint", ms per step from device events.
One JSON line, also written to --out.
    python tools/bench_visibility.py [--batches 1,16,64] [--points 50000] [--steps 10] [--rounds 3] [--out profiles/bench_visibility.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from semantichuman_amd import _lib, editing, ops, scan, synthetic   # noqa: E402
from bench_fit import build                                       # noqa: E402
from bench_scan import time_fit                                   # noqa: E402
from bench_surface import kernels_of                              # noqa: E402

DIRECTIONS = np.array([[-0.33, -0.9, 0.21], [0.55, 0.62, 0.56], [0.8, -0.35, -0.49]])


def viewpoints(x, n, dev):
    """centre + 3 x extent x direction per body, directions cycled."""
    B = x.shape[0]
    lo, hi = x[:, :n].amin(1), x[:, :n].amax(1)
    d = torch.from_numpy(DIRECTIONS[np.arange(B) % 3] / np.linalg.norm(DIRECTIONS, axis=1)[np.arange(B) % 3, None]).float().to(dev)
    return ((lo + hi) / 2 + 3.0 * (hi - lo).amax(1, keepdim=True) * d).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--form", default="planes3")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, _, h = build(dev)
    m.set_compute_dtype(torch.float32)
    _lib.set_f32_mma_mode(a.form)
    n, M = h.sizes[0], a.points
    ft = scan.FaceTable(np.asarray(h.faces, np.int64), n, dev)
    res = {"metric": "vertex_visibility_cost", "model": "semantic 6890", "faces": len(ft), "points": M, "steps": a.steps, "rounds": a.rounds,
           "build_id": _lib.build_id(), "legs": {}}
    med = lambda rows, keys: float(np.median([sum(r.get(k, 0.0) for k in keys) for r in rows]))
    for B in [int(b) for b in a.batches.split(",")]:
        gen = torch.Generator().manual_seed(B)
        z = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        z_kps = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        dummy = editing._default_dummy(m, z)
        with torch.no_grad():                                   # scans as tools/bench_scan.py makes them: nearby bodies, re-sampled with jitter
            x = m.decode(z, z_kps, dummy).contiguous()
            x_t = m.decode(z * 1.1, z_kps, dummy)[:, :n]
            pick = torch.randint(0, n, (B, M), generator=gen).to(dev)
            pts = torch.gather(x_t, 1, pick[:, :, None].expand(-1, -1, 3))
            pts = pts + 0.002 * (x_t.amax((1, 2)) - x_t.amin((1, 2)))[:, None, None] * torch.randn((B, M, 3), generator=gen).to(dev)
            view = viewpoints(x, n, dev)
            xt = torch.from_numpy(synthetic.synth_batch(h.verts, B, seed=3)).to(dev).contiguous()      # body-shaped, with the dummy row
            pick = torch.randint(0, n, (B, M), generator=gen).to(dev)
            st = torch.gather(xt, 1, pick[:, :, None].expand(-1, -1, 3)).contiguous()
            view_t = viewpoints(xt, n, dev)
        scans = scan.ScanBatch(pts, dev)
        scans.viewpoints = view
        del x_t, pick, pts
        vis = ops.vertex_visibility(x, ft.faces, n, view)
        vis_t = ops.vertex_visibility(xt, ft.faces, n, view_t)
        runs = {"plain": [], "grazing": [], "search": [], "decoded": [], "fit": [], "fit_vis": []}
        for _ in range(a.rounds):                               # alternated in one process
            runs["plain"].append(kernels_of(lambda: ops.vertex_visibility(xt, ft.faces, n, view_t)))
            runs["grazing"].append(kernels_of(lambda: scan.visible_vertices(xt, ft, view_t, grazing_angle=80.0)))
            runs["search"].append(kernels_of(lambda: ops.nearest_points(st, xt, nt=n)))
            runs["decoded"].append(kernels_of(lambda: ops.vertex_visibility(x, ft.faces, n, view)))
            runs["fit"].append({"ms": time_fit(m, z, z_kps, dummy, lambda xh: scan.chamfer(xh, scans, None, None, None, 0.5), a.steps)[0]})
            runs["fit_vis"].append({"ms": time_fit(m, z, z_kps, dummy, lambda xh: scan.chamfer(xh, scans, None, None, None, 0.5, visibility="viewpoint",
                                                                                               visibility_faces=ft), a.steps)[0]})
        vk = ("vertex_visibility_kernel", "visibility_fold_kernel")
        p = med(runs["plain"], vk)
        g = med(runs["grazing"], vk + ("vertex_normals_kernel",))
        s = med(runs["search"], ("nearest_search_kernel", "nearest_merge_kernel"))
        fit, fit_vis = med(runs["fit"], ("ms",)), med(runs["fit_vis"], ("ms",))
        res["legs"]["B%d" % B] = {
            "visibility_ms": round(p, 4), "sweep_ms": round(med(runs["plain"], vk[:1]), 4), "fold_ms": round(med(runs["plain"], vk[1:]), 4),
            "with_grazing_ms": round(g, 4), "visible_share": round(float(vis_t.float().mean()), 4), "pairs": B * n * len(ft),
            "decoded_visibility_ms": round(med(runs["decoded"], vk), 4), "decoded_visible_share": round(float(vis.float().mean()), 4),
            "chunks": _lib.load().sh_vertex_visibility_workspace(B, n, len(ft), 0) // (B * n) or 1,
            "scan_search_ms": round(s, 4), "search_pairs": B * n * M, "over_scan_search": round(p / s, 3) if s > 0 else None,
            "fit_step_ms": round(fit, 4), "fit_step_visibility_ms": round(fit_vis, 4), "step_ratio": round(fit_vis / fit, 3) if fit > 0 else None,
            "pass_over_fit_step": round(p / fit, 3) if fit > 0 else None,
            "decoded_pass_over_fit_step": round(med(runs["decoded"], vk) / fit, 3) if fit > 0 else None}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
