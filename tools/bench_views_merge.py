#!/usr/bin/env python3
"""What dropping a rig scan's redundant samples costs and what it saves.  tools/bench_depth.py's ellipsoid at
640 x 480 - ONE body in the rig's frame this time, seen from four sides by tools/bench_views.py's cameras, so that the views
overlap as a real rig's do - at batch 1 / 16 / 64, in one process, the legs alternated over --rounds, medians reported:
  (a) kernel time of the overlap pass and of the three compaction passes, from the library's dispatch events, next to the emit
      pass they follow;
  (b) ScanBatch.from_depth(extrinsics=, merge_tol=) against the same call without merge_tol, from depth tensors on the device to a
      device synchronise (wall clock);
  (c) the kept fraction per body;
  (d) one scan.chamfer(faces=) forward on the merged against the unmerged scans (fewer queries), 6890-vertex template bodies;
  (e) the bytes the overlap pass must move - 25 per live row read (point, normal, view), V - 1 scattered depth words per live
      row, 5 per row written (seen, keep) - its GB/s, and a device copy of the same traffic timed in the same process.
The expectation stated before measuring: the overlap pass costs less than the emit pass it follows.
One JSON line, also written to --out.
    python tools/bench_views_merge.py [--batches 1,16,64] [--rounds 3] [--tol 0.01] [--out profiles/bench_views_merge.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from semantichuman_amd import _lib, scan, synthetic               # noqa: E402
from semantichuman_amd.hierarchy import load_hierarchy            # noqa: E402
from bench_depth import AXES, H, INTR, MAX_STEP, W, Z_CUT, Z_PLANE, copy_ms, wall_ms   # noqa: E402
from bench_surface import kernels_of                              # noqa: E402
from bench_views import V, rig                                    # noqa: E402

OPTS = dict(z_range=(0.1, Z_CUT), max_step=MAX_STEP)


def scene(B, ext, seed=0):
    """One ellipsoid per body near the rig's origin, rendered into its V cameras -> depth float32 [B, V, H, W]; a miss reads
    Z_PLANE, beyond Z_CUT."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1, 1, (B, 3)) * [0.1, 0.05, 0.1]
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    r = np.stack([(u - INTR[2]) / INTR[0], (v - INTR[3]) / INTR[1], np.ones_like(u)], -1)
    D = 1.0 / AXES ** 2
    depth = np.empty((B, V, H, W), np.float32)
    for b in range(B):
        for k in range(V):
            e = ext[b, k].astype(np.float64)
            d, o = r @ e[:, :3].T, e[:, 3] - centres[b]
            qa, qb, qc = (d * d * D).sum(-1), (d * D * o).sum(-1), (o * o * D).sum() - 1.0
            disc = qb * qb - qa * qc
            depth[b, k] = np.where(disc > 0, (-qb - np.sqrt(np.maximum(disc, 0))) / qa, Z_PLANE)
    return depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tol", type=float, default=0.01)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = load_hierarchy(os.path.join(ROOT, "tests", "golden", "template6890.npz"))
    res = {"metric": "views_merge_cost", "image": [H, W], "views": V, "tol": a.tol, "rounds": a.rounds, "build_id": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "legs": {}}
    med = lambda xs: round(float(np.median(xs)), 4)                # noqa: E731
    for B in [int(b) for b in a.batches.split(",")]:
        ext = rig(B)
        depth = torch.from_numpy(scene(B, ext, seed=B)).to(dev).contiguous()
        plain_fn = lambda: scan.ScanBatch.from_depth(depth, INTR, dev, extrinsics=ext, **OPTS)                      # noqa: E731
        merged_fn = lambda: scan.ScanBatch.from_depth(depth, INTR, dev, extrinsics=ext, merge_tol=a.tol, **OPTS)    # noqa: E731
        plain, merged = plain_fn(), merged_fn()
        t = {"plain": [], "merged": []}
        for _ in range(a.rounds):
            t["plain"].append(wall_ms(plain_fn)[0])
            t["merged"].append(wall_ms(merged_fn)[0])
        kern = kernels_of(merged_fn)
        live, rows = int(plain.host_counts.sum()), int(plain.points.shape[0] * plain.points.shape[1])
        frac = merged.host_counts / np.maximum(plain.host_counts, 1)
        nbytes = live * 25 + live * (V - 1) * depth.element_size() + rows * 5
        k_ov, k_emit = kern.get("depth_views_overlap_kernel", 0.0), kern.get("depth_views_emit_kernel", 0.0)
        c_ms = copy_ms(nbytes, dev)
        # (d): template bodies scaled into the ellipsoid's box, so that the searches meet a surface near the scan
        n = h.sizes[0]
        ft = scan.FaceTable(np.asarray(h.faces, np.int64), n, dev)
        x = synthetic.synth_batch(h.verts, B, seed=3)
        lo, hi = x[:, :n].min(1, keepdims=True), x[:, :n].max(1, keepdims=True)
        x = torch.from_numpy(((x - (lo + hi) / 2) / (hi - lo) * (2 * AXES)).astype(np.float32)).to(dev).contiguous()
        ch = {"plain": [], "merged": []}
        with torch.no_grad():
            for name, s in (("plain", plain), ("merged", merged)):
                scan.chamfer(x, s, n=n, faces=ft)
            for _ in range(a.rounds):
                for name, s in (("plain", plain), ("merged", merged)):
                    ch[name].append(wall_ms(lambda: scan.chamfer(x, s, n=n, faces=ft))[0])
        res["legs"]["B%d" % B] = {
            "rows_unmerged": live, "rows_merged": int(merged.host_counts.sum()),
            "kept_fraction": {"mean": round(float(frac.mean()), 4), "min": round(float(frac.min()), 4), "max": round(float(frac.max()), 4)},
            "from_depth_ms": med(t["plain"]), "from_depth_merge_tol_ms": med(t["merged"]),
            "merge_over_plain": round(med(t["merged"]) / med(t["plain"]), 2), "kernels_ms": kern,
            "overlap": {"bytes": nbytes, "kernel_ms": k_ov, "gb_per_s": round(nbytes / k_ov / 1e6, 1) if k_ov > 0 else None,
                        "copy_same_traffic_ms": round(c_ms, 4), "copy_gb_per_s": round(nbytes / c_ms / 1e6, 1),
                        "emit_kernel_ms": k_emit, "overlap_over_emit": round(k_ov / k_emit, 3) if k_emit > 0 else None},
            "compaction_kernels_ms": round(kern.get("scan_compact_count_kernel", 0.0) + kern.get("scan_compact_emit_kernel", 0.0), 4),
            "chamfer_faces_fwd_ms": {"unmerged": med(ch["plain"]), "merged": med(ch["merged"]),
                                     "merged_over_unmerged": round(med(ch["merged"]) / med(ch["plain"]), 3)}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
