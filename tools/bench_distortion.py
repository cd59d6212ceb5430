#!/usr/bin/env python3
"""What lens distortion costs.  The scenes of tools/bench_depth.py at 640 x 480, batch 1 / 16 / 64, every pair in one
process, the legs alternated over --rounds, medians of the kernel times from the library's dispatch events:
  * ScanBatch.from_depth with a ready CameraRays against from_depth without distortion, every pixel kept, one camera and V = 4;
    with the bytes each emit pass must move (the ray form reads 8 more bytes per pixel, plus the halo's share: 18 x 18 rays per
    16 x 16 tile) and the GB/s that makes;
  * the free-space value and gradient on a template body with and without distortion;
  * camera_rays itself.
One JSON line, also written to --out.
    python tools/bench_distortion.py [--batches 1,16,64] [--rounds 3] [--out profiles/bench_distortion.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from semantichuman_amd import _lib, scan                          # noqa: E402
from bench_depth import CENTRE, AXES, H, INTR, W, scene           # noqa: E402

DIST = (5.0, 3.3, 1.0e-4, -5.0e-5, 0.17, 5.3, 4.9, 0.9)            # a rational set of the Azure-Kinect kind
DEV = "cuda:0"
V = 4


def kernel_ms(fn):
    """fn() under the dispatch record -> {kernel name: milliseconds, summed}."""
    _lib.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        out = {}
        for name, _, ms in _lib.profile_records_by_kernel():
            out[name] = out.get(name, 0.0) + ms
    finally:
        _lib.profile_enable(False)
    return out


def median_legs(legs, rounds):
    """{leg: fn} alternated over `rounds` (after one warm-up each) -> {leg: {kernel: median ms}}."""
    for fn in legs.values():
        fn()
    runs = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            runs[k].append(kernel_ms(fn))
    return {k: {name: float(np.median([r.get(name, 0.0) for r in rs])) for name in rs[0]} for k, rs in runs.items()}


def emit_bytes(B, images, rows, rays):
    """The bytes of an emit pass: depth read once, 28 bytes per emitted row (+ 1 for a rig's view), and with a table 8 bytes per
    pixel times (18 / 16)^2 for the halo."""
    pix = B * images * H * W
    return pix * 4 + rows * (28 + (images > 1)) + (int(pix * 8 * (18 / 16) ** 2) if rays else 0)


def body_vertices(B, n=6890, seed=0):
    """A template body: points on the scene's ellipsoids grown by 10 %, so that some stand in free space and some beside the
    silhouette -> float32 [B, n + 1, 3]."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((B, n + 1, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return (CENTRE + 1.1 * AXES * d).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_distortion.json"))
    args = ap.parse_args()
    out = {"what": "bench_distortion", "H": H, "W": W, "V": V, "distortion": DIST, "device": torch.cuda.get_device_name(0), "build": _lib.build_id(),
           "batches": {}}
    rays1 = scan.camera_rays(INTR, DIST, (H, W), DEV)
    raysV = scan.camera_rays(np.tile(np.asarray(INTR, np.float32), (V, 1)), DIST, (H, W), DEV)
    out["camera_rays_ms"] = median_legs({"rays": lambda: scan.camera_rays(INTR, DIST, (H, W), DEV)}, args.rounds)["rays"]
    for B in (int(b) for b in args.batches.split(",")):
        depth = torch.from_numpy(scene(B)[0]).to(DEV)
        rig = depth[:, None].expand(B, V, H, W).contiguous()
        ext = np.broadcast_to(np.eye(4)[:3], (B, V, 3, 4)).copy()
        x = torch.from_numpy(body_vertices(B)).to(DEV).requires_grad_(True)
        fields = {"pinhole": scan.DepthField.from_depth(depth, INTR, z_range=(0.5, 3.5)),
                  "rays": scan.DepthField.from_depth(depth, INTR, z_range=(0.5, 3.5), distortion=rays1)}

        def term(field):
            free, sil = scan.free_space(x, field)
            (free + sil).sum().backward()

        legs = {"one_pinhole": lambda: scan.ScanBatch.from_depth(depth, INTR, DEV),
                "one_rays": lambda: scan.ScanBatch.from_depth(depth, INTR, DEV, distortion=rays1),
                "rig_pinhole": lambda: scan.ScanBatch.from_depth(rig, INTR, DEV, extrinsics=ext),
                "rig_rays": lambda: scan.ScanBatch.from_depth(rig, INTR, DEV, extrinsics=ext, distortion=raysV),
                "term_pinhole": lambda: term(fields["pinhole"]), "term_rays": lambda: term(fields["rays"])}
        ms = median_legs(legs, args.rounds)
        row = {"kernel_ms": ms}
        for leg, images in (("one", 1), ("rig", V)):
            for form in ("pinhole", "rays"):
                k = ms["%s_%s" % (leg, form)]
                emit = next(v for name, v in k.items() if name.endswith("emit_kernel"))
                nbytes = emit_bytes(B, images, B * images * H * W, form == "rays")
                row["%s_%s_emit" % (leg, form)] = {"ms": emit, "bytes": nbytes, "GB_per_s": nbytes / emit / 1e6}
        out["batches"][str(B)] = row
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
