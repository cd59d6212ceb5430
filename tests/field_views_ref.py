"""Host reference of the rig form of the free-space / silhouette term (include/sh_kernels.h, "Free space from a rig"), numpy only
and built on tests/field_ref.py: the model -> camera maps in float64 in the header's order, the transform and the carried-back
gradient in float32 one operation at a time, the per-view case list by field_ref.terms, and a float64 restatement."""
import math

import numpy as np

from tests import field_ref as R

F32 = np.float32
IDENTITY = np.asarray([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F32)


def cameras(pose, ext):
    """pose float32 [12] (A row-major, t) or None, ext float32 [V, 12] (R row-major, t_v) -> cam float32 [V, 12] = (M | c): the
    header's float64 expressions in its order, each word rounded once; NaN rows for a NaN in ext or a det that is 0 or not finite."""
    a = (IDENTITY if pose is None else np.asarray(pose, F32)).astype(np.float64)
    ext = np.asarray(ext, F32)
    rows = [a[0:3], a[3:6], a[6:9]]
    t = a[9:12]
    with np.errstate(all="ignore"):
        k = []
        for r in range(3):
            p, q = rows[(r + 1) % 3], rows[(r + 2) % 3]
            k.append([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]])
        det = (a[0] * k[0][0] + a[1] * k[0][1]) + a[2] * k[0][2]
        inv = [[k[c][i] / det for c in range(3)] for i in range(3)]
        out = np.full(ext.shape, np.nan, F32)
        if det == 0 or not np.isfinite(det):
            return out
        for v, row in enumerate(ext):
            if np.isnan(row).any():
                continue
            e = row.astype(np.float64)
            p = [((inv[i][0] * t[0] + inv[i][1] * t[1]) + inv[i][2] * t[2]) + e[9 + i] for i in range(3)]
            for i in range(3):
                for c in range(3):
                    out[v, 3 * i + c] = F32((e[i] * inv[0][c] + e[3 + i] * inv[1][c]) + e[6 + i] * inv[2][c])
                out[v, 9 + i] = F32(-((e[i] * p[0] + e[3 + i] * p[1]) + e[6 + i] * p[2]))
    return out


def transform(x, cam):
    """Q = M x + c for float32 points [n, 3] and one cam row [12], the header's float32 order."""
    x, cam = np.asarray(x, F32), np.asarray(cam, F32)
    with np.errstate(all="ignore"):
        q = np.stack([((cam[3 * i] * x[:, 0] + cam[3 * i + 1] * x[:, 1]) + cam[3 * i + 2] * x[:, 2]) + cam[9 + i] for i in range(3)], 1)
    assert q.dtype == F32
    return q


def terms(x, n, fields, cam, v_mask=None, margin=0.0):
    """One body: x float32 [rows, 3] in the model's frame, fields: the V field_ref.Field of its cameras, cam float32 [V, 12] ->
    (term float32 [V, n], kind uint8 [V, n], g float32 [V, n, 3] in each camera's frame, counts int32 [V, 4])."""
    per = [R.terms(transform(np.asarray(x, F32)[:n], cam[v]), n, f, v_mask, margin) for v, f in enumerate(fields)]
    return tuple(np.stack([p[j] for p in per]) for j in range(4))


def losses(term, kind, counts):
    """(free, silhouette) of one body: exact sums over vertices and views divided by n_act, float64."""
    n_act = int(counts[0][0])
    if n_act == 0:
        return 0.0, 0.0
    return (math.fsum(term[kind == R.FREE].astype(np.float64)) / n_act, math.fsum(term[kind == R.SILHOUETTE].astype(np.float64)) / n_act)


def gradient(kind, g, counts, gL, rows, cam):
    """g_x float32 [rows, 3] of one body in the model's frame: per view fl(fl(gL[k] * fl(1 / n_act)) * g) carried back by M^T in
    the header's order and added in float32, the views ascending, from zero."""
    out = np.zeros((rows, 3), F32)
    n_act = int(counts[0][0])
    if n_act == 0:
        return out
    inv = F32(1) / F32(n_act)
    n = kind.shape[1]
    with np.errstate(all="ignore"):
        for v in range(kind.shape[0]):
            m = np.asarray(cam[v], F32)
            for k, what in ((0, R.FREE), (1, R.SILHOUETTE)):
                s = F32(gL[k]) * inv
                has = np.nonzero(kind[v] == what)[0]
                w = s * g[v][has]
                back = np.stack([(m[j] * w[:, 0] + m[3 + j] * w[:, 1]) + m[6 + j] * w[:, 2] for j in range(3)], 1)
                assert back.dtype == F32
                out[:n][has] = out[:n][has] + back
    return out


def terms64(x, n, fields, cam, v_mask=None, margin=0.0):
    """The term restated in float64: Q = M x + c with the float32 cam widened, then field_ref.terms64 per view -> (free [V, n],
    silhouette [V, n]) and the number of active vertices."""
    x = np.asarray(x, np.float64)[:n]
    free, sil, n_act = [], [], 0
    for v, f in enumerate(fields):
        m = np.asarray(cam[v], np.float64)
        q = x @ m[:9].reshape(3, 3).T + m[9:]
        fr, si, n_act = R.terms64(q, n, f, v_mask, margin)
        free.append(fr), sil.append(si)
    return np.stack(free), np.stack(sil), n_act


def losses64(x, n, fields, cam, v_mask=None, margin=0.0):
    free, sil, n_act = terms64(x, n, fields, cam, v_mask, margin)
    return (math.fsum(free.ravel()) / n_act, math.fsum(sil.ravel()) / n_act) if n_act else (0.0, 0.0)


def rigid(rng, spread=0.3):
    """A random proper rotation and a translation of size `spread` -> (R [3, 3], t [3]) float64."""
    q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    q = q * np.sign(np.linalg.det(q))
    return q, spread * rng.standard_normal(3)


def pack(Rm, t):
    """(R | t) -> the 12 words, float32."""
    return np.concatenate([np.asarray(Rm, np.float64).reshape(9), np.asarray(t, np.float64)]).astype(F32)
