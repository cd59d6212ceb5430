#!/usr/bin/env python3
"""Time the robust terms against the plain path on the 6890-vertex semantic model (built as tools/bench_fit.py builds it) and
M-point scans, batch 1 / 16 / 64, both directions: one editing.fit_scan step and one scan.align iteration, each robust form
("geman-mcclure", "huber") alternated with robust=None in the same process, plus the per-launch times of the kernels that carry
the penalty (forward, gradient, moments) from the library's dispatch events.  One JSON line, also written to
profiles/bench_robust.json.
    python tools/bench_robust.py [--batches 1,16,64] [--points 50000] [--steps 10] [--rounds 3]"""
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
from bench_align import timed                                     # noqa: E402
from bench_fit import build                                       # noqa: E402

FORMS = (None, "geman-mcclure", "huber")
KERNELS = ("chamfer_fwd", "chamfer_bwd", "align_moments")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--form", default="planes3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_robust.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, _, h = build(dev)
    m.set_compute_dtype(torch.float32)
    _lib.set_f32_mma_mode(a.form)
    n, M = h.sizes[0], a.points
    res = {"metric": "robust_over_plain", "model": "semantic 6890", "points": M, "form": a.form, "steps": a.steps, "rounds": a.rounds,
           "w_model_to_scan": 0.5, "build_id": _lib.build_id(), "legs": {}}
    for B in [int(s) for s in a.batches.split(",")]:
        gen = torch.Generator().manual_seed(B)
        z = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        z_kps = torch.randn((B, 17, 8), generator=gen).to(dev) * 0.5
        dummy = editing._default_dummy(m, z)
        with torch.no_grad():                                   # scans as tools/bench_align.py makes them
            x_t = m.decode(z * 1.1, z_kps, dummy)[:, :n]
            pick = torch.randint(0, n, (B, M), generator=gen).to(dev)
            pts = torch.gather(x_t, 1, pick[:, :, None].expand(-1, -1, 3))
            extent = float((x_t.amax((1, 2)) - x_t.amin((1, 2))).mean())
            pts = pts + 0.002 * extent * torch.randn((B, M, 3), generator=gen).to(dev)
            x0 = m.decode(z, z_kps, dummy)
        scans = scan.ScanBatch(pts, dev)
        del x_t, pick, pts
        sigma = 0.02 * extent

        def kw(form):
            return {} if form is None else dict(robust=form, robust_scale=sigma)

        def fit(form, steps):
            return lambda: editing.fit_scan(m, z, z_kps, scans, steps=steps, lr=1e-3, w_model_to_scan=0.5, dummy=dummy, **kw(form))

        def icp(form, steps):
            return lambda: scan.align(x0, scans, iters=steps, w_model_to_scan=0.5, **kw(form))

        for form in FORMS:                                      # warm-up (allocator, plans, code objects)
            fit(form, 2)(); icp(form, 2)()
        t = {(what, form): [] for what in ("fit", "icp") for form in FORMS}
        for _ in range(a.rounds):                               # alternated in one process
            for form in FORMS:
                t["fit", form].append(timed(fit(form, a.steps), a.steps)[0])
                t["icp", form].append(timed(icp(form, a.steps), a.steps)[0])
        leg = {}
        for form in FORMS:
            _lib.profile_enable(True)
            fit(form, 3)(); icp(form, 3)()
            torch.cuda.synchronize()
            rec = _lib.profile_records_by_kernel()
            _lib.profile_enable(False)
            tag = "" if form is None else "_robust"
            km = {}
            for k in KERNELS:
                ms = [v for name, _, v in rec if name == k + tag + "_kernel"]
                km[k] = round(sum(ms) / len(ms), 5)
            leg[str(form)] = {"fit_scan_step_ms": round(float(np.median(t["fit", form])), 4),
                              "align_iteration_ms": round(float(np.median(t["icp", form])), 4), "kernel_ms_per_launch": km}
        for form in FORMS[1:]:
            for key in ("fit_scan_step_ms", "align_iteration_ms"):
                leg[form][key.replace("_ms", "_over_plain")] = round(leg[form][key] / leg["None"][key], 4)
        res["legs"]["B%d" % B] = leg
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
