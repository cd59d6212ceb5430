#!/usr/bin/env python3
"""What a rig of depth cameras costs as one scan, and what the any-view visibility pass costs.  tools/bench_depth.py's
ellipsoid scene at 640 x 480, V = 4 cameras on a circle around the rig's centre, batch 1 / 16 / 64, in one process, the legs
alternated over --rounds, medians reported:
  (a) ScanBatch.from_depth(depth [B, V, H, W], extrinsics=) against what a user did before it existed: V x from_depth, Pose.apply
      per view, the normals rotated in torch, then concatenated and padded.  Both start from depth tensors on the device and end
      in a device synchronise (wall clock).
  (b) the emit pass of the fused call: the bytes it must move (depth read once, every output written once), kernel time from the
      library's dispatch events, the GB/s that makes, and a device copy of the same traffic timed in the same process.
  (c) sh_vertex_visibility_views at V = 4 on the 6890-vertex template (13 776 faces, synthetic.synth_batch bodies) against four
      calls of sh_vertex_visibility, kernel time from the dispatch events.
One JSON line, also written to --out.
    python tools/bench_views.py [--batches 1,16,64] [--rounds 3] [--out profiles/bench_views.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from semantichuman_amd import _lib, ops, scan, synthetic          # noqa: E402
from semantichuman_amd.hierarchy import load_hierarchy            # noqa: E402
from bench_depth import H, INTR, MAX_STEP, W, Z_CUT, copy_ms, scene, wall_ms   # noqa: E402
from bench_surface import kernels_of                              # noqa: E402
from bench_visibility import viewpoints                           # noqa: E402

V = 4
OPTS = dict(z_range=(0.1, Z_CUT), max_step=MAX_STEP)


def rig(B):
    """V cameras on a circle of radius 2.2 around the rig's origin, each looking at it -> extrinsics float32 [B, V, 3, 4]."""
    ext = np.zeros((V, 3, 4), np.float32)
    for v in range(V):
        a = 2 * np.pi * v / V
        ext[v, :, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        ext[v, :, 3] = ext[v, :, :3] @ np.array([0, 0, -2.2])
    return np.broadcast_to(ext, (B, V, 3, 4)).copy()


def by_hand(depth, ext_poses, rots):
    """What a rig user did before: per view from_depth, the cloud moved with Pose.apply, the normals rotated in torch (Pose.apply
    does not touch them); then concatenated and padded on the host's say-so."""
    B = depth.shape[0]
    parts = []
    for v in range(V):
        s = scan.ScanBatch.from_depth(depth[:, v], INTR, depth.device, **OPTS)
        moved = ext_poses[v].apply(s.points, s.counts)
        parts.append((moved, torch.einsum("bij,bmj->bmi", rots[v], s.normals), s.host_counts))
    counts = np.sum([p[2] for p in parts], 0)
    M = int(counts.max())
    pts = torch.zeros((B, M, 3), device=depth.device)
    nrm = torch.zeros_like(pts)
    for b in range(B):
        at = 0
        for moved, n, c in parts:
            pts[b, at:at + c[b]], nrm[b, at:at + c[b]] = moved[b, :c[b]], n[b, :c[b]]
            at += int(c[b])
    return pts, nrm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = load_hierarchy(os.path.join(ROOT, "tests", "golden", "template6890.npz"))
    res = {"metric": "depth_views_cost", "image": [H, W], "views": V, "rounds": a.rounds, "build_id": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "legs": {}}
    med = lambda xs: round(float(np.median(xs)), 4)
    for B in [int(b) for b in a.batches.split(",")]:
        depth = torch.from_numpy(np.stack([scene(B, seed=10 * B + v)[0] for v in range(V)], 1)).to(dev).contiguous()
        ext = rig(B)
        e = torch.from_numpy(ext).to(dev)
        poses = [scan.Pose(e[:, v, :, :3].contiguous(), e[:, v, :, 3].contiguous(), torch.ones(B)) for v in range(V)]
        rots = [e[:, v, :, :3].contiguous() for v in range(V)]
        fused = lambda: scan.ScanBatch.from_depth(depth, INTR, dev, extrinsics=ext, **OPTS)
        hand = lambda: by_hand(depth, poses, rots)
        s, (hp, _) = fused(), hand()
        assert hp.shape[1] == s.points.shape[1]                  # the same rows, in another order inside a view
        t = {"fused": [], "hand": []}
        for _ in range(a.rounds):
            t["fused"].append(wall_ms(fused)[0])
            t["hand"].append(wall_ms(hand)[0])
        kern = kernels_of(fused)
        m_all = int(s.host_counts.sum())
        nbytes = B * V * H * W * 4 + m_all * (12 + 12 + 4 + 1)
        k_emit = kern.get("depth_views_emit_kernel", 0.0)
        c_ms = copy_ms(nbytes, dev)
        leg = {"points": m_all, "from_depth_extrinsics_ms": med(t["fused"]), "by_hand_ms": med(t["hand"]),
               "by_hand_over_fused": round(med(t["hand"]) / med(t["fused"]), 2), "kernels_ms": kern,
               "emit": {"bytes": nbytes, "kernel_ms": k_emit, "gb_per_s": round(nbytes / k_emit / 1e6, 1) if k_emit > 0 else None,
                        "copy_same_traffic_ms": round(c_ms, 4), "copy_gb_per_s": round(nbytes / c_ms / 1e6, 1)}}
        # (c): the template's bodies, the first camera off the symmetry planes and the others a quarter turn about y further each
        n = h.sizes[0]
        ft = scan.FaceTable(np.asarray(h.faces, np.int64), n, dev)
        x = torch.from_numpy(synthetic.synth_batch(h.verts, B, seed=3)).to(dev).contiguous()
        centre = (x[:, :n].amin(1) + x[:, :n].amax(1)) / 2
        arm = viewpoints(x, n, dev) - centre
        turn = lambda p, k: torch.stack([np.cos(k * np.pi / 2) * p[:, 0] + np.sin(k * np.pi / 2) * p[:, 2], p[:, 1],
                                         -np.sin(k * np.pi / 2) * p[:, 0] + np.cos(k * np.pi / 2) * p[:, 2]], 1)
        views = torch.stack([centre + turn(arm, k) for k in range(V)], 1).float().contiguous()
        singles = [views[:, v].contiguous() for v in range(V)]
        got, bits = ops.vertex_visibility_views(x, ft.faces, n, views, seen=True)
        for v in range(V):
            assert torch.equal((bits >> v) & 1, ops.vertex_visibility(x, ft.faces, n, singles[v]).int())
        rv, rs = [], []
        for _ in range(a.rounds):
            rv.append(sum(kernels_of(lambda: ops.vertex_visibility_views(x, ft.faces, n, views, seen=True)).values()))
            rs.append(sum(kernels_of(lambda: [ops.vertex_visibility(x, ft.faces, n, sv) for sv in singles]).values()))
        leg["visibility"] = {"vertices": n, "faces": len(ft), "views_kernel_ms": med(rv), "four_single_calls_ms": med(rs),
                             "views_over_four_singles": round(med(rv) / med(rs), 3), "visible_share": round(float(got.float().mean()), 4)}
        res["legs"]["B%d" % B] = leg
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
