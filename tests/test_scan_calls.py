"""What scan fitting launches, pinned: for a table of configurations of scan.chamfer, scan.align, editing.fit_scan and
editing.register_scan - every kind of scan -> model partner (vertex, vertex under the vertex-normal gate, surface bounded by the
vertex search, surface under the face-normal gate) against the other arguments that decide which searches run - the ordered list
of (kernel, shape tag) from the library's dispatch record is compared with tests/golden/scan_launches.json, and two runs must
give the same bits.  The fixture was recorded on the MI355X by this file run as a script,

    python -m tests.test_scan_calls --record

at the commit before scan._MatchPlan became the one home of that routing, so it holds what the five hand-written
copies of the rule launched.

The shape tags of the search kernels (`chunks=`) do not depend on the device: the split is a rule over a constant number of
workgroup slots (tests/test_chunk_rule_host.py pins it on the host).  The decoder's convolutions in the editing-level lists size
their grids by the device's compute units, so those lists are the MI355X's.

Shapes are the smallest that still take every route: small_ae.npz, 3 bodies with ragged clouds of at most 63 points and their
normals; the editing level runs the semantic model of test_surface_gated.fit_setup on clouds cut to about 300 points."""
import argparse
import functools
import importlib
import json
import os

import pytest
import torch

import semantichuman_amd
from tests import surface_gated_ref as G
from tests.launch_record import launches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "scan_launches.json")
PARTS = list(range(1, 16))
KINDS = ("vertex", "vertex_gated", "surface", "surface_gated")


def kind_args(kind, faces, trunc, plane=False):
    """The keyword arguments that select a partner kind; plane: the pose step is point-to-plane, which on bare vertex pairs needs
    the triangles for its normals."""
    kw = {"vertex": dict(normal_faces=faces) if plane else {}, "vertex_gated": dict(normal_angle=60, normal_faces=faces),
          "surface": dict(faces=faces), "surface_gated": dict(faces=faces, normal_angle=60, gate_on="surface")}[kind]
    return dict(kw, trunc=trunc)


@functools.lru_cache(maxsize=None)
def scan_data(pkg):
    """(x, FaceTable, ScanBatch with normals, vertex mask) of the small model, made with `pkg`'s classes."""
    x, faces, n, counts, clouds, normals, vmask = G.case_inputs("small_ae.npz", 3, 63, True)
    assert max(counts) <= 63 and len(set(counts)) == 3
    return (torch.as_tensor(x, dtype=torch.float32).to(DEV), pkg.scan.FaceTable(faces, n, DEV), pkg.scan.ScanBatch(clouds, DEV, normals=normals),
            vmask)


@functools.lru_cache(maxsize=None)
def fit_data(pkg):
    """The semantic model, its start latents, the triangles as an array (the editing functions make the table) and clouds of
    about 300 points with normals."""
    from tests.test_surface_gated import fit_setup
    m, z0, z_kps, dummy, x_star, n, faces, clouds, normals, trunc = fit_setup()
    keep = [300 - 11 * b for b in range(len(clouds))]
    sb = pkg.scan.ScanBatch([c[:k] for c, k in zip(clouds, keep)], DEV, order="morton", normals=[c[:k] for c, k in zip(normals, keep)])
    return m, z0, z_kps, dummy, faces, sb, trunc


def chamfer_case(kind, w, record, masked):
    def run(pkg):
        x, ft, sb, vmask = scan_data(pkg)
        xg = x.clone().requires_grad_(True)
        matches = {} if record else None
        loss = pkg.scan.chamfer(xg, sb, vertex_mask=vmask if masked else None, w_model_to_scan=w, matches=matches, **kind_args(kind, ft, 0.1))
        g, = torch.autograd.grad(loss.sum(), xg)
        return [loss.detach(), g, matches]
    run.data = scan_data
    return run


def align_case(kind, step, w, masked, cull=True, iters=2):
    def run(pkg):
        x, ft, sb, vmask = scan_data(pkg)
        return list(pkg.scan.align(x, sb, iters=iters, w_model_to_scan=w, vertex_mask=vmask if masked else None, step=step, cull=cull,
                                   **kind_args(kind, ft, 0.1, step == "plane")))
    run.data = scan_data
    return run


def fit_case(kind):
    def run(pkg):
        m, z0, z_kps, dummy, faces, sb, trunc = fit_data(pkg)
        return list(pkg.editing.fit_scan(m, z0, z_kps, sb, parts=PARTS, steps=2, lr=1e-2, w_model_to_scan=0.5, dummy=dummy,
                                         **kind_args(kind, faces, trunc)))
    run.data = fit_data
    return run


def register_case(kind, align_on, align_step):
    def run(pkg):
        m, z0, z_kps, dummy, faces, sb, trunc = fit_data(pkg)
        return list(pkg.editing.register_scan(m, z0, z_kps, sb, parts=PARTS, mode="rigid", init="identity", align_iters=2, align_every=1, steps=2,
                                              lr=1e-2, w_model_to_scan=0.5, dummy=dummy, align_on=align_on, align_step=align_step,
                                              **kind_args(kind, faces, trunc, align_step == "plane")))
    run.data = fit_data
    return run


CONFIGS = {}
for kind in KINDS:
    for w in (0.0, 0.5):
        for rec in (False, True):
            CONFIGS["chamfer-%s-w%g-matches%d" % (kind, w, rec)] = chamfer_case(kind, w, rec, masked=rec and w > 0)
for kind in KINDS:
    for step in ("point", "plane"):
        for w in (0.0, 1.0):
            CONFIGS["align-%s-%s-w%g" % (kind, step, w)] = align_case(kind, step, w, masked=step == "point" and w > 0)
for kind in ("surface", "surface_gated"):
    CONFIGS["align-%s-point-w1-nocull" % kind] = align_case(kind, "point", 1.0, False, cull=False)
CONFIGS["align-surface_gated-plane-w1-iters0"] = align_case("surface_gated", "plane", 1.0, False, iters=0)
for kind in KINDS:
    CONFIGS["fit-%s" % kind] = fit_case(kind)
for align_on, kinds in (("vertices", KINDS), ("surface", ("surface", "surface_gated"))):      # align_on="surface" needs faces
    for align_step in ("point", "plane"):
        for kind in kinds:
            CONFIGS["register-%s-on_%s-%s" % (kind, align_on, align_step)] = register_case(kind, align_on, align_step)


def tensors(*values):
    """Every tensor in what a configuration returned, in a fixed order: dicts by sorted key, a Pose as (packed, scale, solved), a
    ScanBatch as (points, normals), a FaceTable as its faces; None and plain numbers are left out."""
    out = []
    for v in values:
        if torch.is_tensor(v):
            out.append(v)
        elif isinstance(v, dict):
            out += tensors(*(v[k] for k in sorted(v)))
        elif isinstance(v, (list, tuple)):
            out += tensors(*v)
        elif hasattr(v, "packed"):
            out += tensors(v.packed, v.scale, v.solved)
        elif hasattr(v, "vf_idx"):
            out.append(v.faces)
        elif hasattr(v, "points"):
            out += tensors(v.points, v.normals)
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                                     b.contiguous().reshape(-1).view(torch.uint8))


def record(name, pkg):
    """One configuration under the dispatch record -> (its tensors, ["kernel|shape tag", ...] in launch order).  Its inputs are
    made before the record is switched on: building the model launches too."""
    CONFIGS[name].data(pkg)
    out, rec = launches(lambda: tensors(CONFIGS[name](pkg)))
    return out, ["%s|%s" % kt for kt in rec]


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as fh:
        f = json.load(fh)
    return {name: [f["launches"][i] for i in idx] for name, idx in f["configs"].items()}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_launch_sequence(name):
    first, got = record(name, semantichuman_amd)
    second = tensors(CONFIGS[name](semantichuman_amd))
    assert len(first) == len(second) > 0 and all(same_bits(u, v) for u, v in zip(first, second))
    want = fixture()[name]
    differ = [k for k, (u, v) in enumerate(zip(got, want)) if u != v]
    assert got == want, "%d launches, %d recorded; first difference at %s" % (
        len(got), len(want), [(k, got[k], want[k]) for k in differ[:1]] or min(len(got), len(want)))


def test_the_fixture_covers_the_table():
    assert sorted(fixture()) == sorted(CONFIGS)
    assert all(len(v) > 0 for k, v in fixture().items() if "iters0" not in k)


def main():
    ap = argparse.ArgumentParser(description="record the launch lists of every configuration")
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--package", default="semantichuman_amd", help="the package whose scan and editing modules run")
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    pkg = importlib.import_module(a.package)
    table, configs = {}, {}
    for name in CONFIGS:
        configs[name] = [table.setdefault(s, len(table)) for s in record(name, pkg)[1]]
        print("%-48s %4d launches" % (name, len(configs[name])))
    if a.record:
        with open(a.out, "w") as fh:
            fh.write('{"launches": %s,\n "configs": {\n%s\n}}\n' % (json.dumps(list(table), indent=0), ",\n".join(
                '  %s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in configs.items())))


if __name__ == "__main__":
    main()
