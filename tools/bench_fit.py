#!/usr/bin/env python3
"""Time one step of girth-targeted fitting (editing.fit_latents: decode -> girth objective -> backward to the part latents ->
Adam) on the 6890-vertex semantic model (built as tools/bench_semantic.py builds it), batch 1 / 64 / 1024, in the fp32 forms
planes3 and exact and in bf16; each leg runs the data-only backward (frozen decoder: no weight-gradient launches) and the
forced-full one (stack.FULL_WGRAD: every conv layer's weight gradient computed and discarded), alternated in this process.
Milliseconds per fit step from device events after warm-up.  One JSON line.
    python tools/bench_fit.py [--batches 1,64,1024] [--steps 20] [--rounds 3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import semantichuman_amd as sh                                   # noqa: E402
from semantichuman_amd import _lib, editing, measure, stack       # noqa: E402
from semantichuman_amd import constants as C, synthetic           # noqa: E402
from semantichuman_amd.hierarchy import load_hierarchy            # noqa: E402
from bench_semantic import voronoi_parts                          # noqa: E402


def build(dev):
    h = load_hierarchy(os.path.join(ROOT, "tests", "golden", "template6890.npz"))
    vi = h.verts / np.asarray((0.25, 0.15, 0.9))
    idx = np.arange(h.sizes[0])
    for d in h.D:
        idx = idx[np.asarray(d.col[:-1])]
    coarse = dict(zip(C.PART_LIST, voronoi_parts(vi[idx], 17)))
    torch.manual_seed(2)
    m = sh.SpiralAutoencoder_multiz_partkps(C.KPS_INDEX_LIST, coarse, C.FILTER_SIZES_ENC, C.FILTER_SIZES_DEC, 8, 8, h.sizes,
                                            h.spiral_sizes, h.spirals, h.D, h.U, dev)
    # girth rings: plane cuts of the template at a few heights (oblique normals, as the reference calibrates them)
    f = np.asarray(h.faces)
    edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    lo, hi = h.verts[:, 1].min(), h.verts[:, 1].max()
    fac, epi = [], []
    for t in (0.3, 0.45, 0.6, 0.7):
        p = np.array([0.0, lo + t * (hi - lo), 0.0])
        try:
            fa, ep = measure.ring_from_plane(h.verts, edges, p, np.array([0.05, 1.0, 0.03]))
        except ValueError:
            continue
        fac.append(fa); epi.append(ep)
    return m, measure.GirthRings(fac, epi, dev), h


def time_leg(m, rings, z0, z_kps, dummy, target, steps, full):
    stack.FULL_WGRAD = full

    def objective(x_hat):
        return ((measure.girths(x_hat, rings) - target) / target).pow(2).sum(1)
    editing.fit_latents(m, z0, z_kps, objective, None, steps=3, lr=1e-3, dummy=dummy)           # warm-up (allocator, plans)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    editing.fit_latents(m, z0, z_kps, objective, None, steps=steps, lr=1e-3, dummy=dummy)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--forms", default="planes3,exact,bf16")
    ap.add_argument("--profile-one", action="store_true", help="run a single data-only fit of 5 steps (for rocprofv3) and exit")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, rings, h = build(dev)
    res = {"metric": "fit_step_ms", "model": "semantic 6890", "rings": rings.n_rings, "steps": a.steps, "rounds": a.rounds,
           "build_id": _lib.build_id(), "legs": {}}
    for B in [int(s) for s in a.batches.split(",")]:
        x = torch.from_numpy(synthetic.synth_batch(h.verts, B, seed=1)).to(dev)
        z = torch.randn((B, 17, 8), device=dev) * 0.5
        z_kps = torch.randn((B, 17, 8), device=dev) * 0.5
        dummy = editing._default_dummy(m, z)
        with torch.no_grad():
            target = measure.girths(m.decode(z, z_kps, dummy), rings) * 1.04
        del x
        for form in a.forms.split(","):
            if form == "bf16":
                m.set_compute_dtype(torch.bfloat16)
                _lib.set_f32_mma_mode("exact")
            else:
                m.set_compute_dtype(torch.float32)
                _lib.set_f32_mma_mode(form)
            if a.profile_one:
                editing.fit_latents(m, z, z_kps, lambda xh: measure.girths(xh, rings).sum(1), None, steps=5, lr=1e-3, dummy=dummy)
                torch.cuda.synchronize()
                print(json.dumps({"profile_one": True, "B": B, "form": form}))
                return
            t = {"data_only": [], "full": []}
            for _ in range(a.rounds):                   # alternated in one process
                t["data_only"].append(time_leg(m, rings, z, z_kps, dummy, target, a.steps, False))
                t["full"].append(time_leg(m, rings, z, z_kps, dummy, target, a.steps, True))
            stack.FULL_WGRAD = False
            res["legs"]["B%d_%s" % (B, form)] = {k: round(float(np.median(v)), 4) for k, v in t.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
