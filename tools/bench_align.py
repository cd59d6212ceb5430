#!/usr/bin/env python3
"""Time scan alignment on the 6890-vertex semantic model (built as tools/bench_fit.py builds it) against M-point scans moved by
a similarity, batch 1 / 16 / 64, scan -> model only ("one") and both directions ("both"):
  * one editing.register_scan step with a pose update after every step against one editing.fit_scan step, same process,
    alternated (the pose update reuses the step's matches: three launches, no search);
  * the three launches of a pose update against chamfer_bwd_kernel of the same step, from the library's dispatch events;
  * one scan.align iteration against the same iteration in torch (chunked nearest indices as tools/bench_scan.py forms them,
    torch.linalg.svd on [B, 3, 3]), time and peak allocated bytes.
One JSON line.
    python tools/bench_align.py [--batches 1,16,64] [--points 50000] [--steps 10] [--rounds 3]"""
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
from bench_scan import CHUNK_CELLS                                # noqa: E402

UPDATE_KERNELS = ("align_moments_kernel", "align_solve_kernel", "transform_points_kernel")


def timed(fn, steps):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps, int(torch.cuda.max_memory_allocated())


def torch_icp_iteration(x, s, n, A, t, w):
    """One similarity ICP iteration in torch on full scans (no ragged counts): transform, nearest indices, Umeyama by SVD."""
    B, M = s.shape[0], s.shape[1]
    cur = torch.matmul(s, A.transpose(1, 2)) + t[:, None, :]
    xv = x[:, :n]
    c = max(1, CHUNK_CELLS // (B * n))
    idx_sm = torch.empty((B, M), dtype=torch.int64, device=s.device)
    best = torch.full((B, n), float("inf"), device=s.device)
    idx_ms = torch.zeros((B, n), dtype=torch.int64, device=s.device)
    for c0 in range(0, M, c):
        sc = cur[:, c0:c0 + c]
        d = (sc[:, :, None, 0] - xv[:, None, :, 0]).square_()
        d += (sc[:, :, None, 1] - xv[:, None, :, 1]).square_()
        d += (sc[:, :, None, 2] - xv[:, None, :, 2]).square_()
        idx_sm[:, c0:c0 + c] = d.argmin(2)
        if w > 0:
            v, i = d.min(1)
            take = v < best
            best = torch.where(take, v, best)
            idx_ms = torch.where(take, i + c0, idx_ms)
    p = [cur.double()]
    q = [torch.gather(xv, 1, idx_sm[:, :, None].expand(-1, -1, 3)).double()]
    wt = [torch.full((B, M), 1.0 / M, dtype=torch.float64, device=s.device)]
    if w > 0:
        p.append(torch.gather(cur, 1, idx_ms[:, :, None].expand(-1, -1, 3)).double())
        q.append(xv.double())
        wt.append(torch.full((B, n), w / n, dtype=torch.float64, device=s.device))
    p, q, wt = torch.cat(p, 1), torch.cat(q, 1), torch.cat(wt, 1)
    W = wt.sum(1)
    pb, qb = (p * wt[:, :, None]).sum(1) / W[:, None], (q * wt[:, :, None]).sum(1) / W[:, None]
    pc, qc = p - pb[:, None], q - qb[:, None]
    H = torch.matmul((qc * wt[:, :, None]).transpose(1, 2), pc) / W[:, None, None]
    U, S, Vt = torch.linalg.svd(H)
    sign = torch.sign(torch.linalg.det(torch.matmul(U, Vt)))
    D = torch.diag_embed(torch.stack([torch.ones_like(sign), torch.ones_like(sign), sign], 1))
    Rm = torch.matmul(torch.matmul(U, D), Vt)
    cs = (Rm * H).sum((1, 2)) / ((pc ** 2).sum(-1) * wt).sum(1) * W
    dA = (cs[:, None, None] * Rm).float()
    dt = (qb - torch.matmul(dA.double(), pb[:, :, None])[:, :, 0]).float()
    return torch.matmul(dA, A), torch.matmul(dA, t[:, :, None])[:, :, 0] + dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--form", default="planes3")
    ap.add_argument("--profile-one", type=int, default=0, help="run 3 register_scan steps at this batch, both directions (for rocprofv3), and exit")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, _, h = build(dev)
    m.set_compute_dtype(torch.float32)
    _lib.set_f32_mma_mode(a.form)
    n, M = h.sizes[0], a.points
    res = {"metric": "register_scan_step_ms", "model": "semantic 6890", "points": M, "form": a.form, "steps": a.steps, "rounds": a.rounds,
           "build_id": _lib.build_id(), "legs": {}}
    th = np.deg2rad(10.0)
    Rz = torch.tensor([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    for B in ([a.profile_one] if a.profile_one else [int(s) for s in a.batches.split(",")]):
        gen = torch.Generator().manual_seed(B)
        z = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        z_kps = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        dummy = editing._default_dummy(m, z)
        with torch.no_grad():                                   # scans as tools/bench_scan.py makes them, then moved by a similarity
            x_t = m.decode(z * 1.1, z_kps, dummy)[:, :n]
            pick = torch.randint(0, n, (B, M), generator=gen).to(dev)
            pts = torch.gather(x_t, 1, pick[:, :, None].expand(-1, -1, 3))
            pts = pts + 0.002 * (x_t.amax((1, 2)) - x_t.amin((1, 2)))[:, None, None] * torch.randn((B, M, 3), generator=gen).to(dev)
            x0 = m.decode(z, z_kps, dummy)
        unmoved = scan.ScanBatch(pts, dev)
        away = scan.Pose((0.9 * Rz)[None].expand(B, -1, -1).contiguous(), torch.tensor([[0.05, -0.03, 0.04]]).expand(B, -1).contiguous())
        moved = scan.Pose.from_packed(away.packed.to(dev), away.scale.to(dev)).apply(unmoved)
        del x_t, pick, pts
        if a.profile_one:
            editing.register_scan(m, z, z_kps, moved, steps=3, lr=1e-3, w_model_to_scan=0.5, align_iters=0, dummy=dummy)
            torch.cuda.synchronize()
            print(json.dumps({"profile_one": True, "B": B}))
            return
        for leg, w in (("one", 0.0), ("both", 0.5)):
            def fit(steps):
                return lambda: editing.fit_scan(m, z, z_kps, unmoved, steps=steps, lr=1e-3, w_model_to_scan=w, dummy=dummy)

            def reg(steps):
                return lambda: editing.register_scan(m, z, z_kps, moved, steps=steps, lr=1e-3, w_model_to_scan=w, align_iters=0,
                                                     align_every=1, dummy=dummy)
            fit(2)(); reg(2)()                                  # warm-up (allocator, plans, code objects)
            t = {"fit": [], "reg": []}
            for _ in range(a.rounds):                           # alternated in one process; both include one final evaluation
                t["fit"].append(timed(fit(a.steps), a.steps))
                t["reg"].append(timed(reg(a.steps), a.steps))
            _lib.profile_enable(True)
            reg(3)()
            torch.cuda.synchronize()
            rec = _lib.profile_records_by_kernel()
            _lib.profile_enable(False)
            km = {k: round(sum(ms for name, _, ms in rec if name == k) / sum(1 for name, _, _ in rec if name == k), 5)
                  for k in UPDATE_KERNELS + ("chamfer_bwd_kernel", "nearest_search_kernel")}
            # one ICP iteration: the library against torch
            scan.align(x0, moved, iters=2, w_model_to_scan=w)
            icp = [timed(lambda: scan.align(x0, moved, iters=a.steps, w_model_to_scan=w), a.steps) for _ in range(a.rounds)]
            A0 = torch.eye(3, device=dev)[None].expand(B, -1, -1).contiguous()
            t0 = torch.zeros((B, 3), device=dev)
            with torch.no_grad():
                torch_icp_iteration(x0, moved.points, n, A0, t0, w)
                ticp = [timed(lambda: torch_icp_iteration(x0, moved.points, n, A0, t0, w), 1) for _ in range(a.rounds)]
            res["legs"]["B%d_%s" % (B, leg)] = {
                "fit_scan_step_ms": round(float(np.median([r[0] for r in t["fit"]])), 4),
                "register_scan_step_ms": round(float(np.median([r[0] for r in t["reg"]])), 4),
                "kernel_ms_per_launch": km, "pose_update_ms": round(sum(km[k] for k in UPDATE_KERNELS), 5),
                "align_iteration_ms": round(float(np.median([r[0] for r in icp])), 4), "align_peak_bytes": max(r[1] for r in icp),
                "torch_iteration_ms": round(float(np.median([r[0] for r in ticp])), 4), "torch_peak_bytes": max(r[1] for r in ticp)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
