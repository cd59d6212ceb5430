#!/usr/bin/env python3
"""What matching by normal costs and what it changes.  On the 6890-vertex semantic model (built as tools/bench_fit.py
builds it) against M-point scans that carry normals, batch 1 / 16 / 64, in one process, alternated:
  * nearest_search_gated_kernel against nearest_search_kernel, both directions, and vertex_normals_kernel - kernel times from the
    library's dispatch events, with the VALU issue share of each search as tools/bench_scan.py reports it;
  * a gated fit_scan step (both directions, trunc) against the ungated step, ms per step from device events.
On body-shaped geometry (synthetic.synth_batch bodies of the template, each scanned from its neighbour's surface with that
surface's normals): the share of ungated vertex matches whose two normals differ by more than 60 and by more than 90 degrees.
One JSON line, also written to --out.
    python tools/bench_normals.py [--batches 1,16,64] [--points 50000] [--steps 10] [--rounds 3] [--out profiles/bench_normals.json]"""
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
from bench_scan import VALU_ISSUE_PEAK, VALU_PER_PAIR, time_fit   # noqa: E402
from bench_surface import kernels_of, sample_surface              # noqa: E402

# VALU instructions per (query, target) pair in nearest_search_gated_kernel's inner loop, from the gfx950 ISA: per 8 targets x 4
# queries 64 v_pk_fma_f32 + 48 v_pk_add_f32 + 32 v_pk_mul_f32 (two pairs each) + 64 v_cmp + 96 v_cndmask_b32 + 26 moves / adds
VALU_PER_PAIR_GATED = 330 / 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--angle", type=float, default=60.0)
    ap.add_argument("--form", default="planes3")
    ap.add_argument("--profile-one", type=int, default=0, help="run 3 gated fit steps at this batch, both directions (for rocprofv3), and exit")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, _, h = build(dev)
    m.set_compute_dtype(torch.float32)
    _lib.set_f32_mma_mode(a.form)
    n, M = h.sizes[0], a.points
    ft = scan.FaceTable(h.faces, n, dev)
    cos_min = float(np.cos(np.radians(a.angle)))
    res = {"metric": "normal_gate_cost", "model": "semantic 6890", "points": M, "angle": a.angle, "form": a.form, "steps": a.steps,
           "rounds": a.rounds, "build_id": _lib.build_id(), "valu_per_pair": round(VALU_PER_PAIR, 3),
           "valu_per_pair_gated": round(VALU_PER_PAIR_GATED, 3), "legs": {}}
    for B in ([a.profile_one] if a.profile_one else [int(s) for s in a.batches.split(",")]):
        gen = torch.Generator().manual_seed(B)
        z = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        z_kps = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        dummy = editing._default_dummy(m, z)
        with torch.no_grad():                                   # scans as tools/bench_scan.py makes them, with their source's vertex normals
            x_t = m.decode(z * 1.1, z_kps, dummy).contiguous()
            pick = torch.randint(0, n, (B, M), generator=gen).to(dev)[:, :, None].expand(-1, -1, 3)
            pts = torch.gather(x_t[:, :n], 1, pick)
            pts = pts + 0.002 * (x_t.amax((1, 2)) - x_t.amin((1, 2)))[:, None, None] * torch.randn((B, M, 3), generator=gen).to(dev)
            nrm = torch.gather(scan.vertex_normals(x_t, ft), 1, pick)
            x0 = m.decode(z, z_kps, dummy).contiguous()
            trunc = float(0.25 * (x0.amax() - x0.amin()))
        scans = scan.ScanBatch(pts.cpu().numpy(), dev, normals=nrm.cpu().numpy())
        del x_t, pick, pts, nrm
        gate = dict(normal_angle=a.angle, normal_faces=ft)
        if a.profile_one:
            editing.fit_scan(m, z, z_kps, scans, steps=3, lr=1e-3, w_model_to_scan=0.5, trunc=trunc, dummy=dummy, **gate)
            torch.cuda.synchronize()
            print(json.dumps({"profile_one": True, "B": B}))
            return
        tn = scan.vertex_normals(x0, ft)
        qn = scan._query_normals(tn, x0.shape[1])

        def searches(gated):
            ops.nearest_points(scans.points, x0, q_count=scans.counts, nt=n, gate=(scans.normals, tn, cos_min) if gated else None)
            ops.nearest_points(x0, scans.points, t_count=scans.counts, gate=(qn, scans.normals, cos_min) if gated else None)

        k_plain, k_gated = [], []
        for _ in range(a.rounds):                               # alternated in one process
            k_plain.append(kernels_of(lambda: searches(False)))
            k_gated.append(kernels_of(lambda: searches(True)))
        k_norm = kernels_of(lambda: scan.vertex_normals(x0, ft))
        med = lambda rows, k: float(np.median([r.get(k, 0.0) for r in rows]))
        ms_p, ms_g = med(k_plain, "nearest_search_kernel"), med(k_gated, "nearest_search_gated_kernel")
        pairs = 2 * B * n * M
        t = {"plain": [], "gated": []}
        for _ in range(a.rounds):
            t["plain"].append(time_fit(m, z, z_kps, dummy, lambda x: scan.chamfer(x, scans, None, None, trunc, 0.5), a.steps))
            t["gated"].append(time_fit(m, z, z_kps, dummy, lambda x: scan.chamfer(x, scans, None, None, trunc, 0.5, **gate), a.steps))
        res["legs"]["B%d" % B] = {
            "search_ms_both_directions": {"plain": round(ms_p, 4), "gated": round(ms_g, 4), "ratio": round(ms_g / ms_p, 3) if ms_p > 0 else None},
            "merge_ms": {"plain": round(med(k_plain, "nearest_merge_kernel"), 4), "gated": round(med(k_gated, "nearest_merge_kernel"), 4)},
            "vertex_normals_ms": k_norm.get("vertex_normals_kernel"),
            "pairs": pairs,
            "valu_fraction": {"plain": round(pairs * VALU_PER_PAIR / (ms_p * 1e-3) / VALU_ISSUE_PEAK, 4) if ms_p > 0 else None,
                              "gated": round(pairs * VALU_PER_PAIR_GATED / (ms_g * 1e-3) / VALU_ISSUE_PEAK, 4) if ms_g > 0 else None},
            "fit_step_ms": {"plain": round(float(np.median([r[0] for r in t["plain"]])), 4),
                            "gated": round(float(np.median([r[0] for r in t["gated"]])), 4)},
            "loss0": {"plain": t["plain"][0][2], "gated": t["gated"][0][2]}}
    # what the gate changes on body-shaped geometry: each body scanned from its neighbour's surface, with that surface's normals
    Bb = 16
    gen = torch.Generator().manual_seed(99)
    xt = torch.from_numpy(synthetic.synth_batch(h.verts, Bb, seed=3)).to(dev)
    src = xt.roll(1, 0)[:, :n].contiguous()
    f = ft.faces.long()
    pa, pb, pc = (src[:, f[:, k]] for k in range(3))
    area = torch.linalg.cross(pb - pa, pc - pa)
    fpick = torch.multinomial(area.norm(dim=2).cpu(), M, replacement=True, generator=gen).to(dev)
    r1 = torch.rand((Bb, M), generator=gen).to(dev).sqrt()[:, :, None]
    r2 = torch.rand((Bb, M), generator=gen).to(dev)[:, :, None]
    g3 = lambda v: torch.gather(v, 1, fpick[:, :, None].expand(-1, -1, 3))
    pts = (1 - r1) * g3(pa) + r1 * (1 - r2) * g3(pb) + r1 * r2 * g3(pc)
    sn = torch.nn.functional.normalize(g3(area), dim=2)
    idx, _ = scan.nearest(pts.contiguous(), xt, t_count=[n] * Bb)
    vn = scan.vertex_normals(xt, ft)
    cosang = (torch.gather(vn, 1, idx.long()[:, :, None].expand(-1, -1, 3)) * sn).sum(-1)
    res["bodies"] = {"B": Bb, "points": M, "share_over_60_deg": round(float((cosang < 0.5).float().mean()), 5),
                     "share_over_90_deg": round(float((cosang < 0.0).float().mean()), 5)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
