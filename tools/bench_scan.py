#!/usr/bin/env python3
"""Time one step of fitting to point clouds (editing.fit_scan: decode -> nearest-point search -> Chamfer -> backward to the part
latents -> Adam) on the 6890-vertex semantic model (built as tools/bench_fit.py builds it) against M-point scans, batch 1 / 16 /
64, scan -> model only ("one") and both directions ("both").  Next to each leg the same step with the objective written in torch
(what a user can do without the kernels: nearest indices in fp32 difference form under no_grad, chunked over the scan points so
that it fits, then the differentiable distances through a gather), timed in the same process after the same warm-up, alternated.
Per leg: ms per step from device events, peak allocated bytes of the step, and the kernels' own ms per objective evaluation from
the library's profile hooks (taken in a separate short run).  One JSON line.
    python tools/bench_scan.py [--batches 1,16,64] [--points 50000] [--steps 10] [--rounds 3]"""
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

# VALU instructions per (query, target) pair in nearest_search_kernel's inner loop, from the gfx950 ISA: per 8 targets x 4 queries
# 48 v_pk_add_f32 + 16 v_pk_mul_f32 + 32 v_pk_fma_f32 (two pairs each) + 32 v_cmp_lt_f32 + 64 v_cndmask_b32 + 15 moves / adds
VALU_PER_PAIR = 207 / 32
VALU_ISSUE_PEAK = 256 * 4 * 2.4e9 / 2 * 64                        # lane-instructions / s: a wave64 instruction issues in 2 cycles per SIMD
CHUNK_CELLS = 1 << 28                                             # pair distances the torch objective holds at once (1 GiB of fp32)


def torch_objective(scans, n, w):
    s = scans.points
    B, M = s.shape[0], s.shape[1]

    def objective(x_hat):
        with torch.no_grad():
            xv = x_hat[:, :n]
            c = max(1, CHUNK_CELLS // (B * n))
            idx_sm = torch.empty((B, M), dtype=torch.int64, device=s.device)
            best = torch.full((B, n), float("inf"), device=s.device)
            idx_ms = torch.zeros((B, n), dtype=torch.int64, device=s.device)
            for c0 in range(0, M, c):
                sc = s[:, c0:c0 + c]
                d = (sc[:, :, None, 0] - xv[:, None, :, 0]).square_()
                d += (sc[:, :, None, 1] - xv[:, None, :, 1]).square_()
                d += (sc[:, :, None, 2] - xv[:, None, :, 2]).square_()
                idx_sm[:, c0:c0 + c] = d.argmin(2)
                if w > 0:
                    v, i = d.min(1)
                    take = v < best
                    best = torch.where(take, v, best)
                    idx_ms = torch.where(take, i + c0, idx_ms)
        L = (s - torch.gather(x_hat, 1, idx_sm[:, :, None].expand(-1, -1, 3))).square().sum(-1).mean(1)
        if w > 0:
            L = L + w * (x_hat[:, :n] - torch.gather(s, 1, idx_ms[:, :, None].expand(-1, -1, 3))).square().sum(-1).mean(1)
        return L
    return objective


def time_fit(m, z, z_kps, dummy, objective, steps):
    editing.fit_latents(m, z, z_kps, objective, None, steps=2, lr=1e-3, dummy=dummy)            # warm-up (allocator, plans, code objects)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    _, losses = editing.fit_latents(m, z, z_kps, objective, None, steps=steps, lr=1e-3, dummy=dummy)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps, int(torch.cuda.max_memory_allocated()), float(losses[0])


def kernel_ms(m, z, z_kps, dummy, objective, evals=3):
    """ms per objective evaluation (forward + backward) of the new kernels, from the profile hooks."""
    _lib.profile_enable(True)
    editing.fit_latents(m, z, z_kps, objective, None, steps=evals, lr=1e-3, dummy=dummy)
    torch.cuda.synchronize()
    rec = _lib.profile_records_by_kernel()
    _lib.profile_enable(False)
    out = {}
    for name in ("nearest_search_kernel", "nearest_merge_kernel", "chamfer_fwd_kernel", "chamfer_bwd_kernel"):
        out[name] = round(sum(ms for k, _, ms in rec if k == name) / evals, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--form", default="planes3")
    ap.add_argument("--profile-one", type=int, default=0, help="run 3 HIP fit steps at this batch, both directions (for rocprofv3), and exit")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, _, h = build(dev)
    m.set_compute_dtype(torch.float32)
    _lib.set_f32_mma_mode(a.form)
    n, M = h.sizes[0], a.points
    res = {"metric": "fit_scan_step_ms", "model": "semantic 6890", "points": M, "form": a.form, "steps": a.steps, "rounds": a.rounds,
           "build_id": _lib.build_id(), "valu_per_pair": round(VALU_PER_PAIR, 3), "legs": {}}
    for B in ([a.profile_one] if a.profile_one else [int(s) for s in a.batches.split(",")]):
        gen = torch.Generator().manual_seed(B)
        z = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        z_kps = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        dummy = editing._default_dummy(m, z)
        with torch.no_grad():                                   # scans: the bodies of nearby latents, re-sampled to M points with jitter
            x_t = m.decode(z * 1.1, z_kps, dummy)[:, :n]
            pick = torch.randint(0, n, (B, M), generator=gen).to(dev)
            pts = torch.gather(x_t, 1, pick[:, :, None].expand(-1, -1, 3))
            pts = pts + 0.002 * (x_t.amax((1, 2)) - x_t.amin((1, 2)))[:, None, None] * torch.randn((B, M, 3), generator=gen).to(dev)
        scans = scan.ScanBatch(pts, dev)
        del x_t, pick, pts
        if a.profile_one:
            editing.fit_scan(m, z, z_kps, scans, steps=3, lr=1e-3, w_model_to_scan=0.5, dummy=dummy)
            torch.cuda.synchronize()
            print(json.dumps({"profile_one": True, "B": B}))
            return
        for leg, w in (("one", 0.0), ("both", 0.5)):
            def hip(x_hat, w=w):
                return scan.chamfer(x_hat, scans, None, None, None, w)
            tor = torch_objective(scans, n, w)
            t = {"hip": [], "torch": []}
            for _ in range(a.rounds):                           # alternated in one process
                t["hip"].append(time_fit(m, z, z_kps, dummy, hip, a.steps))
                t["torch"].append(time_fit(m, z, z_kps, dummy, tor, max(2, a.steps // 2)))
            km = kernel_ms(m, z, z_kps, dummy, hip)
            pairs = B * n * M * (2 if w > 0 else 1)
            search_ms = km["nearest_search_kernel"]
            res["legs"]["B%d_%s" % (B, leg)] = {
                "hip_step_ms": round(float(np.median([r[0] for r in t["hip"]])), 4),
                "torch_step_ms": round(float(np.median([r[0] for r in t["torch"]])), 4),
                "hip_peak_bytes": max(r[1] for r in t["hip"]), "torch_peak_bytes": max(r[1] for r in t["torch"]),
                "loss0_hip": t["hip"][0][2], "loss0_torch": t["torch"][0][2],
                "kernel_ms_per_eval": km, "pairs": pairs,
                "search_valu_fraction": round(pairs * VALU_PER_PAIR / (search_ms * 1e-3) / VALU_ISSUE_PEAK, 4) if search_ms > 0 else None}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
