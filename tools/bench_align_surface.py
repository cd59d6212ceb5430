#!/usr/bin/env python3
"""Time point-to-surface alignment on the 6890-vertex semantic model (built as tools/bench_fit.py builds it) against M-point
Morton-sorted scans sampled on a body's surface and moved by a similarity, batch 1 / 16 / 64, scan -> model only ("one") and both
directions ("both"); same process, alternated, kernel times from the library's dispatch events:
  * align_moments_kernel in both instantiations (the vertex form and the surface form), per launch;
  * one scan.align(faces=) iteration against one vertex iteration;
  * one editing.register_scan step with align_on="surface" against align_on="vertices" (both fit with faces=);
  * where both loops end after --iters iterations on noise-free samples of the body's own surface: pose error (the largest
    displacement of a scan point from its true place, over the body's extent) and relative scale error, worst body of the batch.
One JSON line, also written to --out.
    python tools/bench_align_surface.py [--batches 1,16,64] [--points 50000] [--steps 10] [--rounds 3] [--out profiles/bench_align_surface.json]"""
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

KERNELS = ("align_moments_kernel", "align_moments_surface_kernel", "align_solve_kernel", "transform_points_kernel", "nearest_search_kernel",
           "surface_search_kernel")


def sample_surface(x, faces, M, gen):
    """M points per body drawn uniformly by area on the triangles of x [B, n, 3] (torch, on x's device)."""
    f = torch.as_tensor(faces, dtype=torch.int64, device=x.device)
    a, b, c = x[:, f[:, 0]], x[:, f[:, 1]], x[:, f[:, 2]]
    area = torch.linalg.cross(b - a, c - a).norm(dim=2)
    pick = torch.multinomial(area.cpu(), M, replacement=True, generator=gen).to(x.device)[:, :, None].expand(-1, -1, 3)
    r1 = torch.rand((x.shape[0], M, 1), generator=gen).sqrt().to(x.device)
    r2 = torch.rand((x.shape[0], M, 1), generator=gen).to(x.device)
    return (1 - r1) * torch.gather(a, 1, pick) + r1 * (1 - r2) * torch.gather(b, 1, pick) + r1 * r2 * torch.gather(c, 1, pick)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=40)
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
    res = {"metric": "align_surface_iteration_ms", "model": "semantic 6890", "faces": int(faces.shape[0]), "points": M, "form": a.form,
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
            near = sample_surface(m.decode(z * 1.1, z_kps, dummy)[:, :n], faces, M, gen)      # the fit's target: a neighbouring body
            own = sample_surface(x0[:, :n], faces, M, gen)                                     # the recovery's: the body itself
        away = scan.Pose((0.9 * Rz)[None].expand(B, -1, -1).contiguous(), torch.tensor([[0.05, -0.03, 0.04]]).expand(B, -1).contiguous())
        away = scan.Pose.from_packed(away.packed.to(dev), away.scale.to(dev))
        moved = away.apply(scan.ScanBatch(near.cpu().numpy(), dev, order="morton"))
        own_sb = scan.ScanBatch(own.cpu().numpy(), dev, order="morton")
        own_moved = away.apply(own_sb)
        extent = (x0[:, :n].amax(1) - x0[:, :n].amin(1)).amax(1)
        del near, own
        # where the two loops end: the true pose is the inverse of `away`
        truth = away.inverse()
        acc = {}
        for name, f in (("vertices", None), ("surface", ft)):
            pose, al, _ = scan.align(x0, own_moved, mode="similarity", iters=a.iters, w_model_to_scan=0.0, faces=f)
            err = (al.points - own_sb.points).norm(dim=2).amax(1) / extent
            acc[name] = {"pose_error_over_extent": round(float(err.max()), 6),
                         "scale_error": round(float((pose.scale / truth.scale - 1).abs().max()), 6)}
        for leg, w in (("one", 0.0), ("both", 0.5)):
            def reg(on, steps):
                return lambda: editing.register_scan(m, z, z_kps, moved, steps=steps, lr=1e-3, w_model_to_scan=w, align_iters=0, align_every=1,
                                                     dummy=dummy, faces=ft, align_on=on)

            def icp(f, iters):
                return lambda: scan.align(x0, moved, iters=iters, w_model_to_scan=w, faces=f)
            reg("vertices", 2)(); reg("surface", 2)(); icp(None, 2)(); icp(ft, 2)()         # warm-up (allocator, plans, code objects)
            t = {"reg_v": [], "reg_s": [], "icp_v": [], "icp_s": []}
            for _ in range(a.rounds):                                                         # alternated in one process
                t["reg_v"].append(timed(reg("vertices", a.steps), a.steps)[0])
                t["reg_s"].append(timed(reg("surface", a.steps), a.steps)[0])
                t["icp_v"].append(timed(icp(None, a.steps), a.steps)[0])
                t["icp_s"].append(timed(icp(ft, a.steps), a.steps)[0])
            km = kernel_ms(icp(None, 3))
            km.update({k: v for k, v in kernel_ms(icp(ft, 3)).items() if k not in ("align_moments_kernel",)})
            res["legs"]["B%d_%s" % (B, leg)] = {
                "align_iteration_ms": {"vertices": round(float(np.median(t["icp_v"])), 4), "surface": round(float(np.median(t["icp_s"])), 4)},
                "register_scan_step_ms": {"vertices": round(float(np.median(t["reg_v"])), 4), "surface": round(float(np.median(t["reg_s"])), 4)},
                "kernel_ms_per_launch": km, "after_%d_iterations" % a.iters: acc}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
