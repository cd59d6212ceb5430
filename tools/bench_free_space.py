#!/usr/bin/env python3
"""What the depth field and the free-space / silhouette term cost.  The ellipsoid scene of tools/bench_depth.py at
640 x 480, batch 1 / 16 / 64, in one process, the legs alternated over --rounds, medians reported.
  * "field": DepthField.from_depth on images already on the device (z_range cuts the far plane: the body is SURFACE, the rest
    EMPTY) - wall time and kernel time per kernel from the library's dispatch events, the bytes the two passes must move, the
    GB/s that makes, a device copy with the same traffic, and ScanBatch.from_depth on the same images next to it.
  * "fit": a fit step (decode, objective, backward, Adam) of the 6890-vertex semantic model of tools/bench_fit.py against a
    50 000-point scan, with and without the term under a pose that carries the decoded body into the ellipsoid's place; the
    term's two kernels and the share of the step that the rest of it (the pose inverse and the transform, in torch) takes.
One JSON line, also written to --out.
    python tools/bench_free_space.py [--batches 1,16,64] [--rounds 3] [--out profiles/bench_free_space.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from semantichuman_amd import _lib, editing, scan                 # noqa: E402
from bench_depth import AXES, H, INTR, W, Z_CUT, copy_ms, scene, wall_ms   # noqa: E402
from bench_fit import build                                       # noqa: E402
from bench_scan import time_fit                                   # noqa: E402
from bench_surface import kernels_of                              # noqa: E402

FIELD_KERNELS = ("depth_field_column_kernel", "depth_field_row_kernel")
TERM_KERNELS = ("free_space_fwd_kernel", "free_space_bwd_kernel")


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
    res = {"metric": "free_space_cost", "image": [H, W], "model": "semantic 6890", "points": M, "steps": a.steps, "rounds": a.rounds,
           "build_id": _lib.build_id(), "legs": {}}
    med = lambda v: round(float(np.median(v)), 4)
    for B in [int(b) for b in a.batches.split(",")]:
        depth, centres = scene(B, seed=B)
        d_dev = torch.from_numpy(depth).to(dev)
        make = lambda: scan.DepthField.from_depth(d_dev, INTR, dev, z_range=(0.5, Z_CUT))
        as_scan = lambda: scan.ScanBatch.from_depth(d_dev, INTR, dev, z_range=(0.5, Z_CUT))
        field = make()
        as_scan()
        # ---- fit: the decoded bodies, a scan near them, the pose that puts them where the ellipsoid stands
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
            t = (lo + hi) / 2 - s[:, None] * torch.from_numpy(centres).float().to(dev)
        pose = scan.Pose(A, t, s)
        plain = lambda xh: scan.chamfer(xh, scans, None, None, None, 0.5)

        def with_term(xh):
            free, sil = scan.free_space(xh, field, pose=pose)
            return plain(xh) + (free + sil)

        kinds, counts = scan.free_space_kinds(x, field, pose=pose)
        t_field = {k: [] for k in ("field", "scan")}
        k_field, k_term, fit, fit_term = [], [], [], []
        for _ in range(a.rounds):                                                            # alternated in one process
            t_field["field"].append(wall_ms(make)[0])
            t_field["scan"].append(wall_ms(as_scan)[0])
            k_field.append(kernels_of(make, evals=1))
            fit.append(time_fit(m, z, z_kps, dummy, plain, a.steps)[0])
            fit_term.append(time_fit(m, z, z_kps, dummy, with_term, a.steps)[0])
            xg = x.clone().requires_grad_(True)
            k_term.append(kernels_of(lambda: sum(scan.free_space(xg, field, pose=pose)).sum().backward(), evals=1))
        kern = {k: med([r.get(k, 0.0) for r in k_field]) for k in FIELD_KERNELS}
        k_ms = sum(kern.values())
        px = B * H * W
        nbytes = px * (4 + 1 + 4 + 2) + px * (2 + 4)                                         # column pass: depth in, cls / z / candidates out; row pass: candidates in, nearest out
        c_ms = copy_ms(nbytes, dev)
        term = {k: med([r.get(k, 0.0) for r in k_term]) for k in TERM_KERNELS}
        f0, f1 = med(fit), med(fit_term)
        res["legs"]["B%d" % B] = {
            "field": {"from_depth_ms_device_input": med(t_field["field"]), "scanbatch_from_depth_ms": med(t_field["scan"]), "kernels_ms": kern,
                      "kernel_total_ms": round(k_ms, 4), "bytes": nbytes, "gb_per_s": round(nbytes / k_ms / 1e6, 1) if k_ms > 0 else None,
                      "copy_same_traffic_ms": round(c_ms, 4), "copy_gb_per_s": round(nbytes / c_ms / 1e6, 1),
                      "surface_share": round(float((field.cls == 2).float().mean()), 4)},
            "fit": {"fit_step_ms": f0, "fit_step_with_term_ms": f1, "step_ratio": round(f1 / f0, 4) if f0 > 0 else None,
                    "term_kernels_ms": term, "term_kernels_over_step": round(sum(term.values()) / f0, 4) if f0 > 0 else None,
                    "rest_of_term_ms": round(f1 - f0 - sum(term.values()), 4),
                    "counts_active_free_silhouette_outside": counts.sum(0).tolist()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
