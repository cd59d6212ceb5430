#!/usr/bin/env python3
"""What a depth image costs as a scan.  An analytic scene, no renderer and no file: 640 x 480, an ellipsoid of body
proportions in front of a far plane, the depth from ray / quadric intersection on the host; per body the ellipsoid is moved a
little.  Batch 1 / 16 / 64, in one process, the legs alternated over --rounds, medians reported.  Two uses of the same images:
  * "subject": z_range cuts the plane, what remains is the body - a user's scan.  ScanBatch.from_depth against what the same user
    did before it existed: unprojection of the same pixels in numpy, then ScanBatch(clouds, dev, normals="estimate",
    viewpoints=0).  Both start from the depth on the host and end in a device synchronise; from_depth is also timed from a
    depth tensor already on the device.  Also: the angle between the normals and the ellipsoid's analytic ones, grid against the
    k = 16 estimate on the same points, and scan.nearest_surface (kernel time) on the emitted tile order against the same
    points re-sorted with order="morton", on a template body scaled into the ellipsoid's place.
  * "frame": every pixel kept.  The bytes the call must move (depth read once, every output written once), kernel time from the
    library's dispatch events, the GB/s that makes, and a device copy with the same traffic (half the bytes read, half written)
    timed in the same process.
One JSON line, also written to --out.
    python tools/bench_depth.py [--batches 1,16,64] [--rounds 3] [--out profiles/bench_depth.json]"""
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
from semantichuman_amd import _lib, scan, synthetic               # noqa: E402
from semantichuman_amd.hierarchy import load_hierarchy            # noqa: E402
from bench_surface import kernels_of                              # noqa: E402

H, W = 480, 640
INTR = (525.0, 525.0, 319.5, 239.5)
AXES = np.array([0.25, 0.85, 0.15])                               # half-width, half-height, half-depth of the "body", metres
CENTRE = np.array([0.0, 0.0, 2.2])
Z_PLANE, Z_CUT, MAX_STEP = 4.0, 3.5, 0.1


def scene(B, seed=0):
    """-> (depth float32 [B, H, W], the ellipsoids' centres [B, 3])."""
    rng = np.random.default_rng(seed)
    centres = CENTRE + rng.uniform(-1, 1, (B, 3)) * [0.15, 0.05, 0.2]
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    r = np.stack([(u - INTR[2]) / INTR[0], (v - INTR[3]) / INTR[1], np.ones_like(u)], -1)
    D = 1.0 / AXES ** 2
    depth = np.empty((B, H, W), np.float32)
    for b, c in enumerate(centres):
        qa, qb, qc = (r * r * D).sum(-1), (r * D * c).sum(-1), (c * c * D).sum() - 1.0
        disc = qb * qb - qa * qc
        depth[b] = np.where(disc > 0, (qb - np.sqrt(np.maximum(disc, 0))) / qa, Z_PLANE)
    return depth, centres


def numpy_unproject(depth):
    """What a user wrote before from_depth: the pixels below Z_CUT of every image as [m_b, 3] float32 clouds, row-major."""
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    out = []
    for z in depth:
        keep = np.isfinite(z) & (z > 0) & (z <= Z_CUT)
        zz = z[keep]
        out.append(np.stack([(u[keep] - np.float32(INTR[2])) * zz / np.float32(INTR[0]), (v[keep] - np.float32(INTR[3])) * zz / np.float32(INTR[1]), zz], -1))
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def angles_deg(normals, points, counts, centres):
    """Angle of every known normal to the ellipsoid's analytic one at its point -> (median, 90th percentile, known share)."""
    out, known_n, total = [], 0, 0
    for b, m in enumerate(counts):
        p, n = points[b, :m].astype(np.float64), normals[b, :m].astype(np.float64)
        g = (p - centres[b]) / AXES ** 2
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        known = np.abs(n).sum(1) > 0
        out.append(np.degrees(np.arccos(np.clip(np.abs((n[known] * g[known]).sum(1)), 0, 1))))
        known_n, total = known_n + int(known.sum()), total + int(m)
    a = np.concatenate(out)
    return round(float(np.median(a)), 4), round(float(np.percentile(a, 90)), 4), round(known_n / max(total, 1), 5)


def copy_ms(nbytes, dev, reps=20):
    """A device copy whose traffic is nbytes: nbytes / 2 read and as many written."""
    src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = load_hierarchy(os.path.join(ROOT, "tests", "golden", "template6890.npz"))
    n = h.sizes[0]
    ft = scan.FaceTable(np.asarray(h.faces, np.int64), n, dev)
    res = {"metric": "depth_image_cost", "image": [H, W], "rounds": a.rounds, "build_id": _lib.build_id(), "max_step": MAX_STEP, "legs": {}}
    med = lambda v: round(float(np.median(v)), 4)
    for B in [int(b) for b in a.batches.split(",")]:
        depth, centres = scene(B, seed=B)
        d_dev = torch.from_numpy(depth).to(dev)
        subject = dict(z_range=(0.5, Z_CUT), max_step=MAX_STEP)
        new = lambda src: scan.ScanBatch.from_depth(src, INTR, dev, **subject)
        old = lambda clouds: scan.ScanBatch(clouds, dev, normals="estimate", viewpoints=[0.0, 0.0, 0.0])
        frame = lambda: scan.ScanBatch.from_depth(d_dev, INTR, dev, max_step=MAX_STEP)
        new(depth), old(numpy_unproject(depth)), frame()                                     # warm-up: every shape the timed window uses
        t = {k: [] for k in ("new_host", "new_dev", "old_numpy", "old_pack", "frame")}
        frame_k = []
        for _ in range(a.rounds):                                                            # alternated in one process
            t["new_host"].append(wall_ms(lambda: new(depth))[0])
            t["new_dev"].append(wall_ms(lambda: new(d_dev))[0])
            t0 = time.perf_counter()
            clouds = numpy_unproject(depth)
            t["old_numpy"].append((time.perf_counter() - t0) * 1e3)
            t["old_pack"].append(wall_ms(lambda: old(clouds))[0])
            t["frame"].append(wall_ms(frame)[0])
            frame_k.append(kernels_of(frame, evals=1))
        got, built, whole = new(d_dev), old(clouds), frame()
        counts = got.host_counts
        assert counts.tolist() == [len(c) for c in clouds]
        # ---- subject: the ratio, the normals
        old_ms = med(t["old_numpy"]) + med(t["old_pack"])
        leg = {"subject": {"points_per_body": [int(counts.min()), int(counts.max())],
                           "from_depth_ms_host_input": med(t["new_host"]), "from_depth_ms_device_input": med(t["new_dev"]),
                           "numpy_unproject_ms": med(t["old_numpy"]), "scanbatch_estimate_ms": med(t["old_pack"]),
                           "old_over_new": round(old_ms / med(t["new_host"]), 2)}}
        g = angles_deg(got.normals.cpu().numpy(), got.points.cpu().numpy(), counts, centres)
        e = angles_deg(built.normals.cpu().numpy(), built.points.cpu().numpy(), counts, centres)
        leg["subject"]["normal_angle_deg"] = {"grid": {"median": g[0], "p90": g[1], "known": g[2]}, "k16_estimate": {"median": e[0], "p90": e[1], "known": e[2]}}
        # ---- subject: the surface sweep on the emitted order against a Morton re-sort of the same points
        x = torch.from_numpy(synthetic.synth_batch(h.verts, B, seed=3)).to(dev)[:, :n].contiguous()
        lo, hi = x.amin(1, keepdim=True), x.amax(1, keepdim=True)
        x = ((x - 0.5 * (lo + hi)) * (2 * AXES[1] / (hi - lo)[..., 1:2]) + torch.from_numpy(centres).to(dev)[:, None, :]).float().contiguous()
        morton = scan.ScanBatch(clouds, dev, order="morton")
        rowmajor = scan.ScanBatch(clouds, dev)
        sweeps = {"tile_order": got, "morton": morton, "row_major": rowmajor}
        ks = {k: [] for k in sweeps}
        for _ in range(a.rounds):
            for k, s in sweeps.items():
                ks[k].append(sum(kernels_of(lambda: scan.nearest_surface(s.points, x, ft, q_count=s.counts, n=n), evals=1).values()))
        leg["subject"]["nearest_surface_ms"] = {k: med(v) for k, v in ks.items()}
        # ---- frame: bytes, rate, the copy
        m_all, M = int(whole.host_counts.sum()), whole.points.shape[1]
        nbytes = B * H * W * 4 + B * M * 28
        kern = {k: med([r.get(k, 0.0) for r in frame_k]) for k in ("depth_count_kernel", "depth_scan_kernel", "depth_emit_kernel")}
        k_ms = sum(kern.values())
        c_ms = copy_ms(nbytes, dev)
        leg["frame"] = {"points": m_all, "bytes": nbytes, "from_depth_ms_device_input": med(t["frame"]), "kernels_ms": kern,
                        "kernel_total_ms": round(k_ms, 4), "gb_per_s": round(nbytes / k_ms / 1e6, 1) if k_ms > 0 else None,
                        "copy_same_traffic_ms": round(c_ms, 4), "copy_gb_per_s": round(nbytes / c_ms / 1e6, 1)}
        res["legs"]["B%d" % B] = leg
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
