#!/usr/bin/env python3
"""Time the point-to-surface scan fit next to the vertex fit it extends (editing.fit_scan with and without `faces`, scan ->
model only) on the 6890-vertex semantic model (built as tools/bench_fit.py builds it) against M-point scans sampled on the
surface of nearby bodies, batch 1 / 16 / 64, scans packed in Morton order.  Same process, alternated, ms per step from device
events.  Then, from the library's dispatch events: the surface search alone with the cull on and off and with sorted and
unsorted scans, the share of (point, triangle) pairs that reach the region test (the search's own counter) - once on the
decoder's output (the bench model has random weights: its "body" is a crumpled sheet whose triangles all overlap, the worst case
for a cull) and once on body-shaped geometry (synthetic.synth_batch of the template, scans sampled on a neighbour's surface) -,
sh_chamfer_surface_bwd next to chamfer_bwd_kernel, and - at the smallest batch - the same objective in chunked torch (exhaustive
point-to-triangle under no_grad, then the differentiable distance on the chosen faces).  One JSON line.
    python tools/bench_surface.py [--batches 1,16,64] [--points 50000] [--steps 10] [--rounds 3] [--out profiles/bench_surface.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from semantichuman_amd import _lib, editing, ops, scan, synthetic  # noqa: E402
from bench_fit import build                                       # noqa: E402

CHUNK_CELLS = 1 << 24                                             # (point, triangle) pairs the torch objective holds at once


def sample_surface(x, faces, M, gen):
    """[B, M, 3]: M points per body, uniform by area on the triangles of x [B, n, 3] (on the device)."""
    a, b, c = (x[:, faces[:, k]] for k in range(3))
    area = torch.linalg.cross(b - a, c - a).norm(dim=2)
    f = torch.multinomial(area.cpu(), M, replacement=True, generator=gen).to(x.device)
    r1 = torch.rand((x.shape[0], M), generator=gen).to(x.device).sqrt()
    r2 = torch.rand((x.shape[0], M), generator=gen).to(x.device)
    pick = lambda t: torch.gather(t, 1, f[:, :, None].expand(-1, -1, 3))
    return (1 - r1)[:, :, None] * pick(a) + (r1 * (1 - r2))[:, :, None] * pick(b) + (r1 * r2)[:, :, None] * pick(c)


def torch_foot(a, ab, ac, s):
    """Ericson's region test in torch, the form of include/sh_kernels.h: (v, w, d2) for broadcastable triangles and points."""
    ap = s - a
    e11, e12, e22 = (ab * ab).sum(-1), (ab * ac).sum(-1), (ac * ac).sum(-1)
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    d3, d4, d5, d6 = d1 - e11, d2 - e12, d1 - e12, d2 - e22
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    tot = va + vb + vc
    den = torch.where(tot > 0, 1.0 / tot, torch.zeros_like(tot))
    v, w = vb * den, vc * den
    zero, one = torch.zeros_like(v), torch.ones_like(v)
    for cond, nv, nw in (((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0) & (d4 - d3 + d5 - d6 > 0),
                          1 - (d4 - d3) / (d4 - d3 + d5 - d6), (d4 - d3) / (d4 - d3 + d5 - d6)),
                         ((vb <= 0) & (d2 >= 0) & (d6 <= 0) & (d2 - d6 > 0), zero, d2 / (d2 - d6)),
                         ((d6 >= 0) & (d5 <= d6), zero, one),
                         ((vc <= 0) & (d1 >= 0) & (d3 <= 0) & (d1 - d3 > 0), d1 / (d1 - d3), zero),
                         ((d3 >= 0) & (d4 <= d3), one, zero),
                         ((d1 <= 0) & (d2 <= 0), zero, zero)):
        v, w = torch.where(cond, nv, v), torch.where(cond, nw, w)
    v = v.clamp(0, 1)
    w = torch.minimum(w.clamp_min(0), 1 - v)
    r = ap - (v[..., None] * ab + w[..., None] * ac)
    return v, w, (r * r).sum(-1)


def torch_objective(scans, faces, n):
    s = scans.points
    B, M = s.shape[0], s.shape[1]
    fl = faces.long()

    def objective(x_hat):
        with torch.no_grad():
            a = x_hat[:, fl[:, 0]]
            ab, ac = x_hat[:, fl[:, 1]] - a, x_hat[:, fl[:, 2]] - a
            c = max(1, CHUNK_CELLS // (B * fl.shape[0]))
            face = torch.empty((B, M), dtype=torch.int64, device=s.device)
            uv = torch.empty((B, M, 2), device=s.device)
            for c0 in range(0, M, c):
                v, w, d = torch_foot(a[:, None], ab[:, None], ac[:, None], s[:, c0:c0 + c, None, :])
                k = d.argmin(2)
                face[:, c0:c0 + c] = k
                uv[:, c0:c0 + c, 0] = torch.gather(v, 2, k[:, :, None])[:, :, 0]
                uv[:, c0:c0 + c, 1] = torch.gather(w, 2, k[:, :, None])[:, :, 0]
        return (s - scan.closest_points(x_hat, fl, face, uv)).square().sum(-1).mean(1)
    return objective


def time_fit(m, z, z_kps, dummy, objective, steps):
    editing.fit_latents(m, z, z_kps, objective, None, steps=2, lr=1e-3, dummy=dummy)            # warm-up
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    _, losses = editing.fit_latents(m, z, z_kps, objective, None, steps=steps, lr=1e-3, dummy=dummy)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps, float(losses[0])


def kernels_of(fn, evals=3):
    """ms per call of fn, per kernel, from the dispatch events."""
    fn()
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    for _ in range(evals):
        fn()
    torch.cuda.synchronize()
    rec = _lib.profile_records_by_kernel()
    _lib.profile_enable(False)
    out = {}
    for k, _, ms in rec:
        out[k] = out.get(k, 0.0) + ms / evals
    return {k: round(v, 4) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--form", default="planes3")
    ap.add_argument("--torch-batch", type=int, default=1, help="the batch at which the torch objective is timed (0: not at all)")
    ap.add_argument("--profile-one", type=int, default=0, help="run 3 surface fit steps at this batch (for rocprofv3) and exit")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, _, h = build(dev)
    m.set_compute_dtype(torch.float32)
    _lib.set_f32_mma_mode(a.form)
    n, M = h.sizes[0], a.points
    ft = scan.FaceTable(h.faces, n, dev)
    nF = len(ft)
    res = {"metric": "fit_scan_surface_step_ms", "model": "semantic 6890", "faces": nF, "points": M, "form": a.form, "steps": a.steps,
           "rounds": a.rounds, "build_id": _lib.build_id(), "legs": {}}
    for B in ([a.profile_one] if a.profile_one else [int(s) for s in a.batches.split(",")]):
        gen = torch.Generator().manual_seed(B)
        z = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        z_kps = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        dummy = editing._default_dummy(m, z)
        with torch.no_grad():                                   # scans: the SURFACES of the bodies of nearby latents, M samples each
            pts = sample_surface(m.decode(z * 1.1, z_kps, dummy)[:, :n], ft.faces.long(), M, gen).cpu().numpy()
            x0 = m.decode(z, z_kps, dummy).contiguous()
        sorted_scans = scan.ScanBatch(pts, dev, order="morton")
        plain_scans = scan.ScanBatch(pts, dev)

        def surf(x_hat, scans=sorted_scans):
            return scan.chamfer(x_hat, scans, faces=ft)

        def vert(x_hat, scans=sorted_scans):
            return scan.chamfer(x_hat, scans)

        if a.profile_one:
            editing.fit_latents(m, z, z_kps, surf, None, steps=3, lr=1e-3, dummy=dummy)
            torch.cuda.synchronize()
            print(json.dumps({"profile_one": True, "B": B}))
            return
        t = {"surface": [], "vertex": [], "surface_unsorted": []}
        for _ in range(a.rounds):                               # alternated in one process
            t["vertex"].append(time_fit(m, z, z_kps, dummy, vert, a.steps))
            t["surface"].append(time_fit(m, z, z_kps, dummy, surf, a.steps))
            t["surface_unsorted"].append(time_fit(m, z, z_kps, dummy, lambda x_hat: surf(x_hat, plain_scans), a.steps))
        leg = {k + "_step_ms": round(float(np.median([r[0] for r in v])), 4) for k, v in t.items()}
        leg["loss0_surface"], leg["loss0_vertex"] = t["surface"][0][1], t["vertex"][0][1]
        leg["surface_over_vertex"] = round(leg["surface_step_ms"] / leg["vertex_step_ms"], 3)
        # the search alone: bound from the vertex search (not timed here), cull on / off, sorted / unsorted
        search = {}
        for name, scans in (("sorted", sorted_scans), ("unsorted", plain_scans)):
            bound = ops.nearest_points(scans.points, x0, q_count=scans.counts, nt=n)[1]
            stats = torch.zeros(2, dtype=torch.int64, device=dev)
            ops.nearest_surface(scans.points, x0, ft.faces, n, scans.counts, None, bound, stats=stats)
            tested = int(stats[0].item())
            search[name] = {"cull": kernels_of(lambda: ops.nearest_surface(scans.points, x0, ft.faces, n, scans.counts, None, bound)),
                            "region_tests": tested, "swept_again": int(stats[1].item()), "share_of_pairs": round(tested / float(B * M * nF), 6)}
            if name == "sorted":
                search[name]["nocull"] = kernels_of(lambda: ops.nearest_surface(scans.points, x0, ft.faces, n, scans.counts, cull=False), evals=1)
        leg["search_ms"] = search
        # the same search on body-shaped geometry: template bodies, each scanned from its neighbour's surface
        xt = torch.from_numpy(synthetic.synth_batch(h.verts, max(B, 2), seed=3)).to(dev)
        pt = sample_surface(xt.roll(1, 0)[:, :n], ft.faces.long(), M, gen)[:B].cpu().numpy()
        xt = xt[:B].contiguous()
        shaped = {}
        shaped_sorted, shaped_plain = scan.ScanBatch(pt, dev, order="morton"), scan.ScanBatch(pt, dev)
        vmask = torch.from_numpy(np.random.RandomState(7).rand(n) < 0.7).to(dev)       # a partial model: 70 % of the vertices active
        for name, scans, mask in (("sorted", shaped_sorted, None), ("unsorted", shaped_plain, None), ("sorted_masked", shaped_sorted, vmask)):
            bound = ops.nearest_points(scans.points, xt, q_count=scans.counts, t_mask=mask, nt=n)[1]
            stats = torch.zeros(2, dtype=torch.int64, device=dev)
            ops.nearest_surface(scans.points, xt, ft.faces, n, scans.counts, mask, bound, stats=stats)
            shaped[name] = {"cull": kernels_of(lambda: ops.nearest_surface(scans.points, xt, ft.faces, n, scans.counts, mask, bound)),
                            "share_of_pairs": round(int(stats[0].item()) / float(B * M * nF), 6), "swept_again": int(stats[1].item()),
                            "swept_again_share": round(int(stats[1].item()) / float(B * M), 6)}
        shaped["sorted"]["nocull"] = kernels_of(lambda: ops.nearest_surface(shaped_sorted.points, xt, ft.faces, n, shaped_sorted.counts,
                                                                          cull=False), evals=1)
        shaped["sorted"]["vertex_search"] = kernels_of(lambda: ops.nearest_points(shaped_sorted.points, xt, q_count=shaped_sorted.counts, nt=n))
        leg["search_ms_body_shaped"] = shaped
        leg["vertex_search_ms"] = kernels_of(lambda: ops.nearest_points(sorted_scans.points, x0, q_count=sorted_scans.counts, nt=n))

        def both_bwd(objective):
            xg = x0.clone().requires_grad_(True)
            torch.autograd.grad(objective(xg).sum(), xg)
        leg["bwd_ms"] = {"surface_bwd_kernel": kernels_of(lambda: both_bwd(surf)).get("surface_bwd_kernel"),
                         "chamfer_bwd_kernel": kernels_of(lambda: both_bwd(vert)).get("chamfer_bwd_kernel")}
        if B == a.torch_batch:
            leg["torch_step_ms"] = round(time_fit(m, z, z_kps, dummy, torch_objective(sorted_scans, ft.faces, n), 2)[0], 4)
        res["legs"]["B%d" % B] = leg
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
