#!/usr/bin/env python3
"""What estimating scan normals from the cloud costs.  M surface samples of synthetic.synth_batch bodies of the
6890-vertex template, batch 1 / 16 / 64, in one process, alternated, kernel times from the library's dispatch events:
  * cloud_kth_kernel (pass 1), cloud_normals_kernel (pass 2 and the finish) and their sum for k = 8 / 16 / 32;
  * two self-searches sh_nearest_points(q = s, t = s) - the yardstick: the two sweeps stream the same bytes and form the same
    distances, so what the estimate costs beyond them is the list insertion and the fp64 moments;
  * the same estimate in chunked torch (cdist blocks, topk, a masked covariance, torch.linalg.eigh) with its peak memory, at the
    batches of --torch-batches (it is slow).
One JSON line, also written to --out.
    python tools/bench_cloud_normals.py [--batches 1,16,64] [--points 50000] [--rounds 3] [--out profiles/bench_cloud_normals.json]"""
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
from bench_surface import kernels_of, sample_surface              # noqa: E402


def torch_estimate(s, k, rows=2048):
    """k-neighbour PCA normals of s [B, M, 3] in plain torch, `rows` queries at a time: the k nearest by cdist + topk (ties cut
    at k, not kept), covariance about the neighbourhood's mean, eigh.  -> unoriented normals [B, M, 3]."""
    B, M, _ = s.shape
    out = torch.empty_like(s)
    for lo in range(0, M, rows):
        q = s[:, lo:lo + rows]
        idx = torch.cdist(q, s).topk(k, dim=2, largest=False).indices                # [B, rows, k]
        nb = torch.gather(s[:, None].expand(-1, q.shape[1], -1, -1), 2, idx[..., None].expand(-1, -1, -1, 3)).double()
        d = nb - nb.mean(2, keepdim=True)
        out[:, lo:lo + rows] = torch.linalg.eigh(d.transpose(2, 3) @ d)[1][..., 0].float()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--torch-batches", default="1")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--ks", default="8,16,32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = load_hierarchy(os.path.join(ROOT, "tests", "golden", "template6890.npz"))
    n, M = h.sizes[0], a.points
    faces = torch.from_numpy(np.asarray(h.faces, np.int64)).to(dev)
    ks = [int(k) for k in a.ks.split(",")]
    torch_B = {int(b) for b in a.torch_batches.split(",") if b}
    res = {"metric": "cloud_normals_cost", "template": "template6890", "points": M, "rounds": a.rounds, "build_id": _lib.build_id(), "legs": {}}
    med = lambda rows, key: float(np.median([r.get(key, 0.0) for r in rows]))
    for B in [int(b) for b in a.batches.split(",")]:
        gen = torch.Generator().manual_seed(B)
        x = torch.from_numpy(synthetic.synth_batch(h.verts, B, seed=3)).to(dev)[:, :n].contiguous()
        s = sample_surface(x, faces, M, gen).contiguous()
        runs = {k: [] for k in ks}
        selfs = []
        for _ in range(a.rounds):                               # alternated in one process
            for k in ks:
                runs[k].append(kernels_of(lambda: ops.cloud_normals(s, None, k)))
            selfs.append(kernels_of(lambda: (ops.nearest_points(s, s), ops.nearest_points(s, s))))
        two = med(selfs, "nearest_search_kernel") + med(selfs, "nearest_merge_kernel")
        leg = {"two_self_searches_ms": round(two, 4), "pairs_per_sweep": B * M * M, "k": {}}
        for k in ks:
            p1, p2 = med(runs[k], "cloud_kth_kernel"), med(runs[k], "cloud_normals_kernel")
            leg["k"][str(k)] = {"pass1_ms": round(p1, 4), "pass2_ms": round(p2, 4), "total_ms": round(p1 + p2, 4),
                                "over_two_searches": round((p1 + p2) / two, 3) if two > 0 else None}
        if B in torch_B:
            leg["torch"] = {}
            for k in ks:
                torch_estimate(s, k)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ref = torch_estimate(s, k)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1)
                nrm = ops.cloud_normals(s, None, k)[0]
                agree = float(((nrm * ref).sum(-1).abs() > 0.999).float().mean())       # the tie rule and fp32 cdist differ on a few points
                leg["torch"][str(k)] = {"ms": round(ms, 3), "peak_mib": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1),
                                        "over_library": round(ms / leg["k"][str(k)]["total_ms"], 2) if leg["k"][str(k)]["total_ms"] > 0 else None,
                                        "share_within_2.6_deg": round(agree, 5)}
        res["legs"]["B%d" % B] = leg
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
