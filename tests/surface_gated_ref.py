"""Host references for the face-normal gate of the surface search (numpy only): the face normal of include/sh_kernels.h ("Nearest
surface points under a normal gate") in float64 and transcribed to fp32 operation by operation, the exhaustive gated closest-point
search built on surface_ref.foot, the fp32 transcription of the centre bound the culled sweep starts from, surface samples that
carry the normal of the face they came from, the inputs the GPU tests share, and a float64 study of what the gate buys."""
import functools
import os

import numpy as np

from tests import align_ref as A
from tests import surface_ref as S
from tests.normals_ref import angle, dot_f32, nearest_gated_f32
from tests.scan_ref import fma32

# ---------------------------------------------------------------------------------------------- measured constants
#     python -m tests.surface_gated_ref
# prints "face normals: largest angle ..." over the synth_batch bodies of each template (batches of 1, 3 and 4, seed 3) and the
# study's figures; the constants below are those maxima, rounded up.  The kernel is given KERNEL_FACTOR times the angle.
F32_FACE_ANGLE = 2.3e-5     # radians; measured 2.2975e-5 (template6890: a sliver face of the batch of 3; small_ae: 1.39e-7), rounded up
KERNEL_FACTOR = 4.0
MARGIN = float(np.float32(1.0) + np.float32(2.0 ** -10))                   # SH_SURFACE_MARGIN
TEMPLATES = ("template6890.npz", "small_ae.npz")
# The study (study_inputs / study): see test_surface_gated_host.py::test_what_the_gate_buys for what the figures mean.
STUDY_OPPOSED_SHARE = 0.0015      # measured 0.0015 (3 of 2000)
STUDY_ERR_UNGATED = 1.247e-2      # measured 1.24700e-2 of the extent
STUDY_ERR_GATED = 1.245e-2        # measured 1.24461e-2


# ---------------------------------------------------------------------------------------------- face normals
def face_normals_f64(x, faces):
    """Unit face normals in float64, x [n, 3]; zero for a face without area."""
    x = np.asarray(x, np.float64)
    faces = np.asarray(faces, np.int64)
    a, b, c = (x[faces[:, k]] for k in range(3))
    cr = np.cross(b - a, c - a)
    ln = np.sqrt((cr * cr).sum(1, keepdims=True))
    return np.where(ln > 0, cr / np.where(ln > 0, ln, 1.0), 0.0)


def face_normals_f32(x, faces, n=None):
    """The header's face normal, operation for operation: ab = b - a, ac = c - a; every cross component fma(u, v, -(w * z));
    len2 = fma(cz, cz, fma(cy, cy, cx * cx)); c / sqrt(len2) when len2 is positive and finite, else zero; a face with a corner
    outside [0, n) gets zero.  x float32 [rows, 3], n = rows unless given."""
    x = np.asarray(x, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n = x.shape[0] if n is None else int(n)
    inside = ((faces >= 0) & (faces < n)).all(1)
    fc = np.where(inside[:, None], faces, 0)
    a, b, c = (x[fc[:, k]] for k in range(3))
    ab, ac = b - a, c - a
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        cr = np.stack([fma32(ab[:, 1], ac[:, 2], -(ab[:, 2] * ac[:, 1])),
                       fma32(ab[:, 2], ac[:, 0], -(ab[:, 0] * ac[:, 2])),
                       fma32(ab[:, 0], ac[:, 1], -(ab[:, 1] * ac[:, 0]))], 1).astype(np.float32)
        len2 = fma32(cr[:, 2], cr[:, 2], fma32(cr[:, 1], cr[:, 1], cr[:, 0] * cr[:, 0]))
        ok = (len2 > 0) & np.isfinite(len2) & inside
        ln = np.sqrt(len2).astype(np.float32)                              # float32 sqrt and division: correctly rounded
        return np.where(ok[:, None], cr / np.where(ok, ln, np.float32(1))[:, None], np.float32(0)).astype(np.float32)


def measure_f32_angle(batches=(1, 3, 4), seed=3):
    """The largest angle between the fp32 transcription's and the float64 face normals, per template, over the synth_batch
    bodies normals_ref.bodies(name, B) for every B of `batches` - 1 and 3 are the batches the GPU test runs, 4 the one the vertex
    normals were measured on (no face of these bodies is without area)."""
    from tests.normals_ref import bodies
    worst = {}
    for name in TEMPLATES:
        w = 0.0
        for B in batches:
            x, f = bodies(name, B, seed)
            n = x.shape[1] - 1
            for b in range(B):
                n32, n64 = face_normals_f32(x[b, :n], f), face_normals_f64(x[b, :n], f)
                assert (np.abs(n32).sum(1) > 0).all() and (np.abs(n64).sum(1) > 0).all()
                w = max(w, float(angle(n32, n64).max()))
        worst[name] = w
    return worst


# ---------------------------------------------------------------------------------------------- the gated search
def cos_min_of(degrees):
    """The gate's threshold as the library's callers form it: cos of the angle in float64, -inf at exactly 180."""
    return -np.inf if float(degrees) == 180.0 else float(np.cos(np.radians(float(degrees))))


def pair_d2_f32(q, verts, faces, cells=1 << 19):
    """surface_ref.foot's fp32 d2 of EVERY (point, face) pair, [nq, nF] float32 - the part of the gated search that does not
    depend on the gate, for callers that ask at several angles."""
    q, verts = np.asarray(q, np.float32), np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64)
    nq, nF = q.shape[0], faces.shape[0]
    out = np.empty((nq, nF), np.float32)
    fb = min(nF, 512) or 1
    qb = max(1, cells // fb)
    Av, Bv, Cv = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    for q0 in range(0, nq, qb):
        for lo in range(0, nF, fb):
            out[q0:q0 + qb, lo:lo + fb] = S.foot(Av[None, lo:lo + fb], Bv[None, lo:lo + fb], Cv[None, lo:lo + fb], q[q0:q0 + qb, None, :], True)[2]
    return out


def closest_gated_from(d_all, q, qn, verts, faces, cos_min, allowed=None):
    """closest_gated (fp32) from the pairs' distances of pair_d2_f32: the gate and the target rule select, the first minimum of a
    row is the lowest face, and the weights of the chosen face are formed once more by the same expression."""
    q, verts, qn = np.asarray(q, np.float32), np.asarray(verts, np.float32), np.asarray(qn, np.float32)
    faces = np.asarray(faces, np.int64)
    ok = np.ones(faces.shape[0], bool) if allowed is None else np.asarray(allowed, bool)[faces].all(1)
    comp = dot_f32(qn[:, None, :], face_normals_f32(verts, faces)[None, :, :]) >= np.float32(cos_min)
    d = np.where(ok[None, :] & comp, d_all, np.float32(np.inf))
    k = d.argmin(1)
    best = d[np.arange(d.shape[0]), k]
    has = best < np.inf
    f = faces[k]
    v, w, dd = S.foot(verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]], q, True)
    assert np.array_equal(dd[has], best[has])
    return np.where(has, k, -1), best, np.where(has[:, None], np.stack([v, w], 1), np.float32(0)).astype(np.float32)


def closest_gated(q, qn, verts, faces, cos_min, allowed=None, f32=True, fn=None, cells=1 << 19):
    """The exhaustive gated search: surface_ref.foot over every (point, face) pair, a pair allowed iff the face is a target
    (`allowed` [n] bool marks the active vertices) and compatible: the fp32 dot of scan_ref.fma32 against float32(cos_min) for
    f32=True (the kernel's answer on the host), the float64 dot otherwise.  Lexicographic minimum of (d2, face); none: face -1,
    d2 inf, uv 0.  fn: the face normals (default: face_normals_f32 / face_normals_f64 of verts)."""
    dt = np.float32 if f32 else np.float64
    q, verts = np.asarray(q, dt), np.asarray(verts, dt)
    faces = np.asarray(faces, np.int64)
    if fn is None:
        fn = face_normals_f32(verts, faces) if f32 else face_normals_f64(verts, faces)
    qn, fn = np.asarray(qn, dt), np.asarray(fn, dt)
    nq, nF = q.shape[0], faces.shape[0]
    ok = np.ones(nF, bool) if allowed is None else np.asarray(allowed, bool)[faces].all(1)
    best = np.full(nq, np.inf, dt)
    bi = np.full(nq, -1, np.int64)
    bv, bw = np.zeros(nq, dt), np.zeros(nq, dt)
    fb = min(nF, 512) or 1
    qb = max(1, cells // fb)
    Av, Bv, Cv = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    for q0 in range(0, nq, qb):
        qs = q[q0:q0 + qb, None, :]
        r = np.arange(qs.shape[0])
        sl = slice(q0, q0 + qb)
        for lo in range(0, nF, fb):
            v, w, d = S.foot(Av[None, lo:lo + fb], Bv[None, lo:lo + fb], Cv[None, lo:lo + fb], qs, f32)
            if f32:
                comp = dot_f32(qn[sl, None, :], fn[None, lo:lo + fb, :]) >= np.float32(cos_min)
            else:
                comp = (qn[sl, None, :] * fn[None, lo:lo + fb, :]).sum(-1) >= cos_min
            d = np.where(ok[None, lo:lo + fb] & comp, d, dt(np.inf))
            k = d.argmin(1)                                                # the lowest face of the block on a tie
            dk = d[r, k]
            take = dk < best[sl]                                           # strict: an earlier block's face wins a tie
            best[sl] = np.where(take, dk, best[sl])
            bi[sl] = np.where(take, lo + k, bi[sl])
            bv[sl], bw[sl] = np.where(take, v[r, k], bv[sl]), np.where(take, w[r, k], bw[sl])
    return bi, best, np.stack([bv, bw], 1)


def centres_f32(verts, faces):
    """The sphere centre of the header's step (1), operation for operation: m = a + (ab + ac) * fl(1 / 3), component-wise, no
    contraction.  verts float32 [n, 3]."""
    x = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64)
    a, b, c = (x[faces[:, k]] for k in range(3))
    third = np.float32(1.0) / np.float32(3.0)
    return (a + ((b - a) + (c - a)) * third).astype(np.float32)


def centre_bound_f32(q, qn, verts, faces, cos_min, allowed=None):
    """The bound the culled gated sweep starts from, on the host: the gated nearest search (normals_ref.nearest_gated_f32) over
    the centres of the target faces, the fp32 face normals as the targets' normals.  -> d2 float32 [nq], +inf where no target
    face is compatible."""
    faces = np.asarray(faces, np.int64)
    ok = None if allowed is None else np.asarray(allowed, bool)[faces].all(1)
    return nearest_gated_f32(np.asarray(q, np.float32), centres_f32(verts, faces), np.asarray(qn, np.float32),
                             face_normals_f32(verts, faces), cos_min, ok)[1]


# ---------------------------------------------------------------------------------------------- inputs
def sample_surface_faces(verts, faces, m, seed, sigma=0.0):
    """surface_ref.sample_surface that also tells where each sample came from: (points float32 [m, 3], face int64 [m]).  The
    noise is added after the face is drawn, so a scan can carry the normal of its source face."""
    rs = np.random.RandomState(seed)
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64)
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    f = rs.choice(faces.shape[0], size=int(m), p=area / area.sum())
    r1, r2 = np.sqrt(rs.rand(int(m))), rs.rand(int(m))
    p = (1 - r1)[:, None] * a[f] + (r1 * (1 - r2))[:, None] * b[f] + (r1 * r2)[:, None] * c[f]
    if sigma:
        p = p + sigma * rs.randn(int(m), 3)
    return p.astype(np.float32), f


def pack_normals_f32(nrm):
    """What scan.pack_normals makes of float64 rows: normalised in float64, rounded to fp32 once, zero rows kept."""
    from semantichuman_amd.scan import pack_normals
    return pack_normals([nrm], [nrm.shape[0]], nrm.shape[0])[0]


@functools.lru_cache(maxsize=None)
def case_inputs(template, B, M, masked, seed=3, flip=True):
    """The inputs of one case of the GPU tests: surface_ref.case_inputs' bodies, face table, counts and vertex mask; the clouds
    are noisy samples (sigma 0.01) of body (b + 1) % B's surface, each carrying the float64 normal of its source face on that
    body.  flip: every fourth normal (j % 4 == 1) is negated and every 29th (j % 29 == 7) zeroed.  -> (x, faces, n, counts,
    clouds, normals, vmask); normals as ScanBatch(normals=) takes them (float64 rows)."""
    x, faces, n, counts, _, vmask = S.case_inputs(template, B, M, masked, "s01", seed)
    clouds, normals = [], []
    for b, m in enumerate(counts):
        src = x[(b + 1) % B, :n]
        p, f = sample_surface_faces(src, faces, m, seed=1000 * seed + 17 * b + M, sigma=0.01)
        nr = face_normals_f64(src, faces)[f]
        if flip:
            j = np.arange(m)
            nr[j % 4 == 1] *= -1.0
            nr[j % 29 == 7] = 0.0
        clouds.append(p)
        normals.append(nr)
    return x, faces, n, counts, clouds, normals, vmask


@functools.lru_cache(maxsize=None)
def case_reference(template, B, M, masked, degrees):
    """closest_gated (fp32) of every body of case_inputs at `degrees`: a list of (face, d2, uv), computed once and shared."""
    x, faces, n, counts, clouds, normals, vmask = case_inputs(template, B, M, masked)
    c = cos_min_of(degrees)
    d_all = _case_pair_d2(template, B, M)
    return [closest_gated_from(d_all[b], clouds[b], pack_normals_f32(normals[b]), x[b, :n], faces, c, vmask) for b in range(B)]


@functools.lru_cache(maxsize=2)
def _case_pair_d2(template, B, M):
    x, faces, n, counts, clouds, normals, vmask = case_inputs(template, B, M, False)     # neither x nor the clouds depend on the mask
    return [pair_d2_f32(clouds[b], x[b, :n], faces) for b in range(B)]


@functools.lru_cache(maxsize=None)
def case_ungated(template, B, M, masked):
    """The ungated answer (surface_ref.closest_f32's) of every body of case_inputs, from the shared pair distances."""
    return case_reference(template, B, M, masked, 180.0)                   # the open gate (the host test holds it against closest_f32)


def check_conditions(template, B, M, masked, degrees=60.0):
    """Asserts that a case is not vacuous (for M >= 63): over its bodies, at `degrees`, at least half the live points keep a
    partner, at least one has none, and at least one partner differs from the ungated one.  -> (kept, none, differing)."""
    ref, ung = case_reference(template, B, M, masked, degrees), case_ungated(template, B, M, masked)
    kept = sum(int((r[0] >= 0).sum()) for r in ref)
    none = sum(int((r[0] < 0).sum()) for r in ref)
    differ = sum(int(((r[0] >= 0) & (r[0] != u[0])).sum()) for r, u in zip(ref, ung))
    assert 2 * kept >= kept + none and none >= 1 and differ >= 1, (template, B, M, masked, kept, none, differ)
    return kept, none, differ


SHAPES = ((1, 1), (3, 63), (3, 1000))
ANGLES = (30.0, 60.0, 90.0, 180.0)


# ---------------------------------------------------------------------------------------------- the study
def study_inputs(template="small_ae.npz", m=2000, shift=0.03, seed=11):
    """One synth_batch body (scan_ref.model_points(v, 1, seed=3)), m noise-free samples of its surface with their source faces'
    float64 normals, moved by a translation of `shift` times the body's extent along align_ref.SHIFT_DIR - a few centimetres on a
    body 1.7 m tall, enough for a sample on the inside of an arm or a thigh to lie nearer to the neighbouring part.
    -> (verts float64 [n, 3], faces, scan float64 [m, 3], normals float64 [m, 3], the true model-frame points, extent)."""
    from semantichuman_amd.hierarchy import load_hierarchy
    from tests import scan_ref
    h = load_hierarchy(os.path.join(os.path.dirname(__file__), "golden", template))
    v, faces = np.asarray(h.verts, np.float64), np.asarray(h.faces, np.int64)
    xb = scan_ref.model_points(v, 1, seed=3)[0, :v.shape[0]].astype(np.float64)
    p, f = sample_surface_faces(xb, faces, m, seed=seed)
    pts = p.astype(np.float64)
    extent = float((xb.max(0) - xb.min(0)).max())
    d = A.SHIFT_DIR / np.linalg.norm(A.SHIFT_DIR)
    return xb, faces, pts + shift * extent * d, face_normals_f64(xb, faces)[f], pts, extent


def icp_surface_gated(x, faces, s, sn, degrees, iters=10, trunc=None):
    """float64 rigid point-to-surface ICP from the identity: the loop of align_surface_ref.icp_surface, scan -> model only, with
    the partner the gated closest point (degrees=None: ungated) and pairs farther than trunc, or without a partner, dropped.
    The scan's normals follow the rotation.  -> (A, t)."""
    x, s, sn = np.asarray(x, np.float64), np.asarray(s, np.float64), np.asarray(sn, np.float64)
    At, t = np.eye(3), np.zeros(3)
    c = -np.inf if degrees is None else cos_min_of(degrees)
    for _ in range(iters):
        cur = A.apply(At, t, s)
        face, d2, uv = closest_gated(cur, sn @ At.T, x, faces, c, f32=False)
        keep = (face >= 0) & (np.isfinite(d2) if trunc is None else d2 < trunc * trunc)
        if keep.sum() < 3:
            break
        qpts = S.rebuild_f64(x, faces, face[keep], uv[keep])
        dA, dt, _, _ = A.umeyama(A.moments(cur[keep], qpts, np.full(int(keep.sum()), 1.0 / len(s)))[0], "rigid")
        At, t = A.compose(dA, dt, At, t)
    return At, t


def study(iters=10, degrees=60.0):
    """-> dict: `opposed` the share of UNGATED float64 foot points of the moved scan that land on a face whose normal opposes
    the sample's by more than 90 degrees; `err_ungated` / `err_gated` the largest displacement of a scan point from its true
    position, as a fraction of the extent, after `iters` rigid surface ICP iterations without / with the gate (trunc = 0.1
    extent on both sides, so that a point without a compatible face is dropped exactly as the library drops it)."""
    xb, faces, s, sn, pts, extent = study_inputs()
    face, _, _ = S.closest_f64(s, xb, faces)
    opposed = float(((sn * face_normals_f64(xb, faces)[face]).sum(1) < 0).mean())
    out = dict(opposed=opposed, extent=extent)
    for key, deg in (("err_ungated", None), ("err_gated", degrees)):
        At, t = icp_surface_gated(xb, faces, s, sn, deg, iters, trunc=0.1 * extent)
        out[key] = float(np.sqrt(((A.apply(At, t, s) - pts) ** 2).sum(1).max())) / extent
    return out


def _measure():
    w = measure_f32_angle()
    for k, v in w.items():
        print("face normals %-18s largest angle fp32 transcription vs float64: %.3e rad" % (k, v), flush=True)
    print("face normals: largest angle %.3e (F32_FACE_ANGLE recorded %.3e)" % (max(w.values()), F32_FACE_ANGLE), flush=True)
    r = study()
    print("study: %.5f of the ungated foot points land on a face opposed by more than 90 degrees; pose error after the loop %.4g of the "
          "extent without the gate, %.4g with it (ratio %.3g)" % (r["opposed"], r["err_ungated"], r["err_gated"],
                                                                   r["err_gated"] / max(r["err_ungated"], 1e-300)), flush=True)


if __name__ == "__main__":
    _measure()
