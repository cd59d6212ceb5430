"""Host references for the nearest-point / Chamfer tests (numpy only): the header's fp32 distance expression mirrored bit for
bit, float64 nearest points chunked over the targets, and the seeded model / scan point sets the tests share."""
import numpy as np

from semantichuman_amd import synthetic

REL = 1e-5          # derived, not measured: the difference form carries at most a few units of 6e-8 per term
EXEMPT_CAP = 1e-3   # share of queries rule (c) may exempt


def fma32(a, b, c):
    """fp32 fused multiply-add of float32 arrays, exactly rounded.  a * b is exact in float64 (24 + 24 bits); the sum with c is
    rounded to float64 to ODD (TwoSum gives the rounding error's sign), and a value rounded to odd at 53 bits rounds to the same
    float32 as the exact one (53 >= 24 + 2; Boldo & Melquiond, "Emulation of a FMA and correctly rounded sums")."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def d2_f32(q, t):
    """include/sh_kernels.h: dx = qx - tx (fp32) ...; d2 = fma(dz, dz, fma(dy, dy, dx * dx)).  q, t broadcastable [..., 3] float32."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    dx, dy, dz = (q[..., k] - t[..., k] for k in range(3))
    return fma32(dz, dz, fma32(dy, dy, dx * dx))


def _blocks(nq, nt, cells=1 << 20):
    """(query block, target block) sizes so that one block of pair values stays cache-sized."""
    tb = min(nt, 1024)
    return max(1, cells // max(tb, 1)), tb


def nearest_f32(q, t, allowed=None):
    """The kernel's answer computed on the host: (idx, d2) of the lexicographic minimum of (d2_f32, i)."""
    nq, nt = q.shape[0], t.shape[0]
    best = np.full(nq, np.inf, np.float32)
    bi = np.full(nq, -1, np.int64)
    qb, tb = _blocks(nq, nt)
    for q0 in range(0, nq, qb):
        qs = q[q0:q0 + qb]
        r = np.arange(qs.shape[0])
        for lo in range(0, nt, tb):
            d = d2_f32(qs[:, None, :], t[None, lo:lo + tb, :])
            if allowed is not None:
                d = np.where(allowed[None, lo:lo + tb], d, np.float32(np.inf))
            k = d.argmin(1)
            dk = d[r, k]
            take = dk < best[q0:q0 + qb]
            best[q0:q0 + qb] = np.where(take, dk, best[q0:q0 + qb])
            bi[q0:q0 + qb] = np.where(take, lo + k, bi[q0:q0 + qb])
    return bi, best


def nearest_f64(q, t, allowed=None):
    """float64: (argmin - lowest index on ties, best d2, second-best DISTINCT d2) per query, in cache-sized blocks."""
    q, t = q.astype(np.float64), t.astype(np.float64)
    nq, nt = q.shape[0], t.shape[0]
    best = np.full(nq, np.inf)
    second = np.full(nq, np.inf)
    bi = np.full(nq, -1, np.int64)
    qb, tb = _blocks(nq, nt)
    for q0 in range(0, nq, qb):
        qs = q[q0:q0 + qb]
        r = np.arange(qs.shape[0])
        sl = slice(q0, q0 + qb)
        for lo in range(0, nt, tb):
            ts = t[lo:lo + tb]
            d = np.subtract.outer(qs[:, 0], ts[:, 0])
            d *= d
            for k in (1, 2):
                e = np.subtract.outer(qs[:, k], ts[:, k])
                e *= e
                d += e
            if allowed is not None:
                d[:, ~allowed[lo:lo + tb]] = np.inf
            k = d.argmin(1)
            dk = d[r, k]
            d[d <= dk[:, None]] = np.inf                                   # what is left: values distinct from (above) the block's best
            rest = d.min(1)
            cand = np.stack([best[sl], second[sl], dk, rest], 1)
            new_best = cand.min(1)
            new_second = np.where(cand > new_best[:, None], cand, np.inf).min(1)
            take = dk < best[sl]
            bi[sl] = np.where(take, lo + k, bi[sl])
            best[sl], second[sl] = new_best, new_second
    return bi, best, second


def check_against_f64(q, t, idx, d2, allowed=None):
    """Rules (a)-(c) of the search test for one body; returns the number of queries rule (c) exempted."""
    idx = np.asarray(idx, np.int64)
    assert (idx >= 0).all() and (idx < t.shape[0]).all()
    if allowed is not None:
        assert allowed[idx].all()
    got = d2_f32(q, t[idx])
    assert np.array_equal(got.view(np.int32), np.asarray(d2, np.float32).view(np.int32)), "(a) d2 is not the header's expression at idx"
    i64, best, second = nearest_f64(q, t, allowed)
    assert (np.asarray(d2, np.float64) <= best * (1 + REL)).all(), "(b)"
    clear = second > best * (1 + REL)
    assert (idx[clear] == i64[clear]).all(), "(c)"
    return int((~clear).sum())


def model_points(verts, B, seed):
    """[B, V + 1, 3] float32: synth_batch bodies with the dummy row."""
    return synthetic.synth_batch(verts, B, seed=seed)


def make_scans(x, n, counts, seed):
    """Scan b = the vertices of body (b + 1) % B plus Gaussian jitter of 1 % of that body's extent, re-sampled with replacement to
    counts[b] points.  x [B, rows, 3]; returns a list of [m_b, 3] float32."""
    rs = np.random.RandomState(seed)
    out = []
    for b, m in enumerate(counts):
        src = x[(b + 1) % x.shape[0], :n].astype(np.float64)
        extent = (src.max(0) - src.min(0)).max()
        pts = src + 0.01 * extent * rs.randn(n, 3)
        out.append(pts[rs.randint(0, n, size=int(m))].astype(np.float32))
    return out
