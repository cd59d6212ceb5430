#!/usr/bin/env python3
"""What the face-normal gate of the surface search costs.  On the 6890-vertex semantic model (built as
tools/bench_fit.py builds it) against M-point scans sampled on a neighbouring decode's surface that carry their source face's
normal (Morton order), batch 1 / 16 / 64, in one process, alternated:
  * face_normals_kernel, the centre pre-pass (nearest_search_gated_kernel over nF centres), surface_search_gated_kernel and the
    other gated launches against the ungated faces= launches (the vertex search that bounds them included) - kernel times from the
    library's dispatch events;
  * a gated fit_scan step (gate_on="surface", trunc) against the ungated faces= step, ms per step from device events;
  * the share of points the finishing kernel swept again, and the region tests per point, from the `stats` counters.
One JSON line, also written to --out.
    python tools/bench_surface_gated.py [--batches 1,16,64] [--points 50000] [--steps 10] [--rounds 3] [--out profiles/bench_surface_gated.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from semantichuman_amd import _lib, editing, ops, scan           # noqa: E402
from bench_fit import build                                       # noqa: E402
from bench_surface import kernels_of, time_fit                    # noqa: E402


def sample_with_normals(x, faces, M, gen):
    """(points [B, M, 3], unit normals [B, M, 3]): M points per body uniform by area on the triangles of x [B, n, 3], each with
    the normal of the face it was drawn on."""
    a, b, c = (x[:, faces[:, k]] for k in range(3))
    cr = torch.linalg.cross(b - a, c - a)
    f = torch.multinomial(cr.norm(dim=2).cpu(), M, replacement=True, generator=gen).to(x.device)
    r1 = torch.rand((x.shape[0], M), generator=gen).to(x.device).sqrt()
    r2 = torch.rand((x.shape[0], M), generator=gen).to(x.device)
    pick = lambda t: torch.gather(t, 1, f[:, :, None].expand(-1, -1, 3))
    p = (1 - r1)[:, :, None] * pick(a) + (r1 * (1 - r2))[:, :, None] * pick(b) + (r1 * r2)[:, :, None] * pick(c)
    return p, torch.nn.functional.normalize(pick(cr), dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--angle", type=float, default=60.0)
    ap.add_argument("--form", default="planes3")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, _, h = build(dev)
    m.set_compute_dtype(torch.float32)
    _lib.set_f32_mma_mode(a.form)
    n, M = h.sizes[0], a.points
    ft = scan.FaceTable(h.faces, n, dev)
    nF = len(ft)
    cos_min = float(np.cos(np.radians(a.angle)))
    res = {"metric": "surface_gate_cost", "model": "semantic 6890", "faces": nF, "points": M, "angle": a.angle, "form": a.form,
           "steps": a.steps, "rounds": a.rounds, "build_id": _lib.build_id(), "legs": {}}
    med = lambda rows, k: round(float(np.median([r.get(k, 0.0) for r in rows])), 4)
    for B in [int(s) for s in a.batches.split(",")]:
        gen = torch.Generator().manual_seed(B)
        z = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        z_kps = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        dummy = editing._default_dummy(m, z)
        with torch.no_grad():
            x_t = m.decode(z * 1.1, z_kps, dummy).contiguous()
            pts, nrm = sample_with_normals(x_t[:, :n], ft.faces.long(), M, gen)
            x0 = m.decode(z, z_kps, dummy).contiguous()
            trunc = float(0.25 * (x0.amax() - x0.amin()))
        scans = scan.ScanBatch(pts.cpu().numpy(), dev, order="morton", normals=nrm.cpu().numpy())
        del x_t, pts, nrm
        fn = ops.face_normals(x0, ft.faces, n)

        def plain():
            d2v = ops.nearest_points(scans.points, x0, q_count=scans.counts, nt=n)[1]
            return ops.nearest_surface(scans.points, x0, ft.faces, n, scans.counts, None, d2v)

        def gated():
            ops.face_normals(x0, ft.faces, n, out=fn)
            return ops.nearest_surface(scans.points, x0, ft.faces, n, scans.counts, gate=(scans.normals, fn, cos_min))

        k_plain, k_gated = [], []
        for _ in range(a.rounds):                               # alternated in one process
            k_plain.append(kernels_of(plain))
            k_gated.append(kernels_of(gated))
        stats = {}
        for key, g in (("plain", None), ("gated", (scans.normals, fn, cos_min))):
            st = torch.zeros(2, dtype=torch.int64, device=dev)
            bound = ops.nearest_points(scans.points, x0, q_count=scans.counts, nt=n)[1] if g is None else None
            face = ops.nearest_surface(scans.points, x0, ft.faces, n, scans.counts, None, bound, stats=st, gate=g)[0]
            tested, again = (int(v) for v in st.cpu())
            stats[key] = {"region_tests_per_point": round(tested / float(B * M), 3), "swept_again_share": round(again / float(B * M), 6),
                          "without_face_share": round(float((face < 0).float().mean()), 6)}
        t = {"plain": [], "gated": []}
        gate = dict(normal_angle=a.angle, gate_on="surface")
        for _ in range(a.rounds):
            t["plain"].append(time_fit(m, z, z_kps, dummy, lambda x: scan.chamfer(x, scans, None, None, trunc, 0.0, faces=ft), a.steps))
            t["gated"].append(time_fit(m, z, z_kps, dummy, lambda x: scan.chamfer(x, scans, None, None, trunc, 0.0, faces=ft, **gate), a.steps))
        names_p = ("nearest_search_kernel", "nearest_merge_kernel", "surface_prep_kernel", "surface_search_kernel", "surface_finish_kernel")
        names_g = ("face_normals_kernel", "surface_prep_gated_kernel", "nearest_search_gated_kernel", "nearest_merge_kernel",
                   "surface_search_gated_kernel", "surface_finish_gated_kernel")
        sum_p = round(sum(med(k_plain, k) for k in names_p), 4)
        sum_g = round(sum(med(k_gated, k) for k in names_g), 4)
        res["legs"]["B%d" % B] = {
            "kernel_ms": {"plain": {k: med(k_plain, k) for k in names_p}, "gated": {k: med(k_gated, k) for k in names_g}},
            "search_ms_total": {"plain": sum_p, "gated": sum_g, "ratio": round(sum_g / sum_p, 3) if sum_p > 0 else None},
            "stats": stats,
            "fit_step_ms": {"plain": round(float(np.median([r[0] for r in t["plain"]])), 4),
                            "gated": round(float(np.median([r[0] for r in t["gated"]])), 4)},
            "loss0": {"plain": t["plain"][0][1], "gated": t["gated"][0][1]}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
