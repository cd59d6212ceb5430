"""Host references for the normal tests (numpy only): the vertex-to-face incidence listed by brute force, area-weighted vertex
normals in float64, the header's fp32 expression mirrored operation for operation on scan_ref.fma32, the gate's fp32 dot
product, and the gated search built on scan_ref.nearest_f32.

`python -m tests.normals_ref` measures F32_ANGLE: the largest angle between the fp32 transcription and float64 over synth_batch
bodies of both templates.  It is a property of the EXPRESSION in fp32 (differences, cross products and a short sum), not of any
kernel; a kernel is held to KERNEL_FACTOR times it, the project's factor for a kernel over its transcription."""
import os

import numpy as np

from semantichuman_amd import synthetic
from semantichuman_amd.hierarchy import load_hierarchy
from tests.scan_ref import fma32, nearest_f32

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TEMPLATES = ("template6890.npz", "small_ae.npz")
F32_ANGLE = 1.41e-6     # radians; measured by `python -m tests.normals_ref` (4 bodies per template, seed 3): 1.409e-6, rounded up
KERNEL_FACTOR = 4.0


def template(name):
    """(verts float64 [n, 3], faces int64 [nF, 3]) of a golden template."""
    h = load_hierarchy(os.path.join(GOLD, name))
    return np.asarray(h.verts, np.float64), np.asarray(h.faces, np.int64)


def bodies(name, B, seed=3):
    """synth_batch bodies with the dummy row, float32 [B, n + 1, 3], and the template's faces."""
    v, f = template(name)
    return synthetic.synth_batch(v, B, seed=seed), f


def incidence_brute(faces, n):
    """For every vertex the list of faces that name it, in ascending face order - by looking at every face."""
    out = [[] for _ in range(n)]
    for f, tri in enumerate(np.asarray(faces)):
        for v in tri:
            out[int(v)].append(f)
    return out


def csr(faces, n):
    """The same as (ptr, idx) arrays."""
    lists = incidence_brute(faces, n)
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    return ptr, np.asarray([f for l in lists for f in l], np.int64)


def normals_f64(x, faces):
    """Area-weighted unit vertex normals in float64; x [n, 3]; zero where the sum vanishes."""
    x = np.asarray(x, np.float64)
    a, b, c = (x[faces[:, k]] for k in range(3))
    cr = np.cross(b - a, c - a)
    s = np.zeros_like(x)
    for k in range(3):
        np.add.at(s, faces[:, k], cr)
    ln = np.sqrt((s * s).sum(1, keepdims=True))
    return np.where(ln > 0, s / np.where(ln > 0, ln, 1.0), 0.0)


def normals_f32(x, faces):
    """include/sh_kernels.h, "Vertex normals", operation for operation: ab = b - a, ac = c - a; every cross component
    fma(u, v, -(w * z)); the components summed in fp32 in ascending face order; len2 = fma(sz, sz, fma(sy, sy, sx * sx));
    s / sqrt(len2) when len2 is positive and finite, else zero.  x float32 [n, 3]."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    a, b, c = (x[faces[:, k]] for k in range(3))
    ab, ac = b - a, c - a
    cr = np.stack([fma32(ab[:, 1], ac[:, 2], -(ab[:, 2] * ac[:, 1])),
                   fma32(ab[:, 2], ac[:, 0], -(ab[:, 0] * ac[:, 2])),
                   fma32(ab[:, 0], ac[:, 1], -(ab[:, 1] * ac[:, 0]))], 1)
    ptr, idx = csr(faces, n)
    deg = np.diff(ptr)
    s = np.zeros((n, 3), np.float32)
    for k in range(int(deg.max()) if n else 0):                            # the k-th face of every vertex that has one: fp32 adds in order
        v = np.nonzero(deg > k)[0]
        s[v] = s[v] + cr[idx[ptr[v] + k]]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        len2 = fma32(s[:, 2], s[:, 2], fma32(s[:, 1], s[:, 1], s[:, 0] * s[:, 0]))
        ok = (len2 > 0) & np.isfinite(len2)
        ln = np.sqrt(len2)                                                 # float32 sqrt and division: correctly rounded
        return np.where(ok[:, None], s / np.where(ok, ln, np.float32(1))[:, None], np.float32(0)).astype(np.float32)


def angle(a, b):
    """The angle between unit vectors, row by row, in float64 (the atan2 form: accurate for tiny angles)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 2.0 * np.arctan2(np.linalg.norm(a - b, axis=-1), np.linalg.norm(a + b, axis=-1))


def dot_f32(qn, tn):
    """The gate's product: fma(qnz, tnz, fma(qny, tny, qnx * tnx)) in fp32; broadcastable [..., 3] float32."""
    qn, tn = np.asarray(qn, np.float32), np.asarray(tn, np.float32)
    return fma32(qn[..., 2], tn[..., 2], fma32(qn[..., 1], tn[..., 1], qn[..., 0] * tn[..., 0]))


def nearest_gated_f32(q, t, qn, tn, cos_min, allowed=None):
    """The gated kernel's answer on the host: scan_ref.nearest_f32 with the per-pair `allowed` = (target allowed) and
    (dot_f32 >= cos_min), one query at a time (nearest_f32 takes one row of allowed targets)."""
    ok = dot_f32(qn[:, None, :], tn[None, :, :]) >= np.float32(cos_min)
    if allowed is not None:
        ok &= np.asarray(allowed, bool)[None, :]
    idx = np.full(q.shape[0], -1, np.int64)
    d2 = np.full(q.shape[0], np.inf, np.float32)
    for j in range(q.shape[0]):
        i, d = nearest_f32(q[j:j + 1], t, ok[j])
        idx[j], d2[j] = i[0], d[0]
    return idx, d2


def unit_normals(rs, shape, zero_share=0.05):
    """Random unit float32 normals [*shape, 3], rounded once from float64, with a share of exact zero rows."""
    v = rs.randn(*shape, 3)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    v[rs.rand(*shape) < zero_share] = 0.0
    return v.astype(np.float32)


def measure_f32_angle(B=4, seed=3):
    worst = {}
    for name in TEMPLATES:
        x, f = bodies(name, B, seed)
        n = x.shape[1] - 1
        worst[name] = max(float(angle(normals_f32(x[b, :n], f), normals_f64(x[b, :n], f)).max()) for b in range(B))
    return worst


if __name__ == "__main__":
    w = measure_f32_angle()
    for k, v in w.items():
        print("%-18s largest angle fp32 transcription vs float64: %.3e rad" % (k, v))
    print("F32_ANGLE (recorded) = %.3e; measured maximum = %.3e" % (F32_ANGLE, max(w.values())))
