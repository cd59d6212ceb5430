"""Float64 references and input builders of tests/test_semantic_kernels.py: the grouped per-part layers, the part pair-distance
loss and the small loss kernels of the semantic loop, restated in plain numpy / torch on the CPU from the same fp32 inputs.

Nothing here touches the GPU; tests/test_semantic_kernels.py checks these functions on the host (against the oracle, which
tests/test_semantic.py pins to the reference) before any kernel is compared with them."""
import numpy as np
import torch

U32 = 2.0 ** -24          # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------- grouped linear
def gate_ratio(got, ref, mag, nr):
    """Worst |got - ref| / ((nr + 2) * 2^-24 * mag) over the elements, and their number.  `mag` is the float64 sum of the
    products' magnitudes (plus |bias|), `nr` the number of products (a scalar or an array).  An fp32 sum of nr products, as one
    FMA chain or as 64 shorter chains joined by a six-level butterfly, with one more rounding for the bias, stays within
    gamma_(nr+1) * mag < (nr + 2) * 2^-24 * mag for every nr used here (nr * 2^-24 < 1e-3).  Where mag is 0 every term is 0 and
    the result must be exactly the reference."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    bound = (np.asarray(nr, dtype=np.float64) + 2.0) * U32 * mag
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    return (float(ratio.max()) if ratio.size else 0.0), int(ratio.size)


def glin_fwd_ref(x, x_off, ws, bs, y_cols, y_off):
    """y[:, y_off[g] : +N_g] = x[:, x_off[g] : +K_g] @ W_g.T + b_g in float64 -> (ref, mag, nr, covered), each [M, y_cols]."""
    xd = x.double().numpy()
    M = xd.shape[0]
    ref, mag = np.zeros((M, y_cols)), np.zeros((M, y_cols))
    nr, cov = np.zeros((M, y_cols)), np.zeros((M, y_cols), dtype=bool)
    for g, w in enumerate(ws):
        N, K = w.shape
        xg, wd = xd[:, x_off[g]:x_off[g] + K], w.double().numpy()
        assert xg.shape[1] == K
        r, m = xg @ wd.T, np.abs(xg) @ np.abs(wd).T
        if bs is not None and bs[g] is not None:
            b = bs[g].double().numpy()
            r, m = r + b, m + np.abs(b)
        sl = slice(y_off[g], y_off[g] + N)
        assert not cov[:, sl].any() and y_off[g] + N <= y_cols
        ref[:, sl], mag[:, sl], nr[:, sl], cov[:, sl] = r, m, K, True
    return ref, mag, nr, cov


def glin_bwd_data_ref(dy, y_off, ws, x_cols, x_off):
    """dx[:, x_off[g] : +K_g] = dy[:, y_off[g] : +N_g] @ W_g in float64 -> (ref, mag, nr, covered), each [M, x_cols]."""
    dd = dy.double().numpy()
    M = dd.shape[0]
    ref, mag = np.zeros((M, x_cols)), np.zeros((M, x_cols))
    nr, cov = np.zeros((M, x_cols)), np.zeros((M, x_cols), dtype=bool)
    for g, w in enumerate(ws):
        N, K = w.shape
        dg, wd = dd[:, y_off[g]:y_off[g] + N], w.double().numpy()
        assert dg.shape[1] == N
        sl = slice(x_off[g], x_off[g] + K)
        assert not cov[:, sl].any() and x_off[g] + K <= x_cols
        ref[:, sl], mag[:, sl], nr[:, sl], cov[:, sl] = dg @ wd, np.abs(dg) @ np.abs(wd), N, True
    return ref, mag, nr, cov


def glin_bwd_wgt_ref(dy, y_off, x, x_off, shapes):
    """Per group (dW = dy_g.T @ x_g, its magnitude sum, db = dy_g.sum(0), its magnitude sum) in float64; shapes: [(N, K)]."""
    dd, xd = dy.double().numpy(), x.double().numpy()
    out = []
    for g, (N, K) in enumerate(shapes):
        dg, xg = dd[:, y_off[g]:y_off[g] + N], xd[:, x_off[g]:x_off[g] + K]
        assert dg.shape[1] == N and xg.shape[1] == K
        out.append((dg.T @ xg, np.abs(dg).T @ np.abs(xg), dg.sum(0), np.abs(dg).sum(0)))
    return out


def glin_inputs(M, shapes, seed, x_gap=0, y_gap=0, x_lead=0, y_lead=0, x_align=1):
    """Random fp32 inputs of one grouped call: groups of (N, K) side by side in x and y, `x_gap` / `y_gap` unused columns behind
    every group, `x_lead` / `y_lead` in front of the first; every x block starts at a multiple of `x_align` past x_lead and the
    row lengths are rounded up to a multiple of 4 -> dict(x, dy, ws, bs, x_off, y_off, x_cols, y_cols)."""
    gen = torch.Generator().manual_seed(seed)
    x_off, y_off, xo, yo = [], [], x_lead, y_lead
    for N, K in shapes:
        xo = x_lead + -(-(xo - x_lead) // x_align) * x_align
        x_off.append(xo); y_off.append(yo)
        xo += K + x_gap; yo += N + y_gap
    x_cols, y_cols = -(-xo // 4) * 4, -(-yo // 4) * 4
    return dict(x=torch.randn(M, x_cols, generator=gen), dy=torch.randn(M, y_cols, generator=gen),
                ws=[torch.randn(N, K, generator=gen) / max(K, 1) ** 0.5 for N, K in shapes],
                bs=[torch.randn(N, generator=gen) for N, K in shapes], x_off=x_off, y_off=y_off, x_cols=x_cols, y_cols=y_cols,
                shapes=list(shapes), M=M)


# ---------------------------------------------------------------------------------------------- part pair-distance loss
def lattice_points(n, rng, jitter=0.2):
    """n points, one per cell of a unit lattice (cells in random order), each moved by at most `jitter` along every axis: no two
    are closer than 1 - 2 * jitter."""
    m = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    while m ** 3 < n:
        m += 1
    cells = rng.permutation(m ** 3)[:n]
    p = np.stack([cells // (m * m), (cells // m) % m, cells % m], 1).astype(np.float64)
    return p + rng.uniform(-jitter, jitter, size=(n, 3))


def pairdist_inputs(sizes, B, N1, seed, s_part=None, noise=8e-3, unsorted=True, thr=0.8, angle_safe_max=200):
    """Synthetic disjoint parts and meshes for the pair loss: part p has sizes[p] vertices of a jittered unit lattice (no two
    closer than 0.6) at scattered rows of an [B, N1, 3] mesh, the reconstruction is x_gt * s_part[p] + uniform noise of at most
    `noise` per coordinate.  With |s_part - 1| = 0.05 (the default alternates 0.95 / 1.05) a pair's reconstructed distance
    differs from s * d by at most 2 sqrt(3) noise <= 0.0462 * 0.6 <= 0.0462 d, so the sign of every term is that of s - 1 with a
    margin of 1.5e-3: the loss has no ambiguous sign by construction.  -> dict(parts, x_gt, x_rec, kps, skl_list, s_part) as
    fp32 tensors / lists."""
    rng = np.random.default_rng(seed)
    P, nv = len(sizes), int(sum(sizes))
    assert nv <= N1
    rows = rng.permutation(N1)[:nv] if unsorted else np.arange(nv)
    parts, o = [], 0
    for n in sizes:
        parts.append(rows[o:o + n].astype(np.int64)); o += n
    s_part = np.asarray([0.95 if p % 2 == 0 else 1.05 for p in range(P)] if s_part is None else s_part, dtype=np.float64)
    x_gt = rng.uniform(-1, 1, size=(B, N1, 3))
    x_rec = rng.uniform(-1, 1, size=(B, N1, 3))
    for p, idx in enumerate(parts):
        for b in range(B):
            x_gt[b, idx] = lattice_points(len(idx), rng) + rng.uniform(-3, 3, size=3)
    x_gt = x_gt.astype(np.float32)
    for p, idx in enumerate(parts):
        x_rec[:, idx] = x_gt[:, idx].astype(np.float64) * s_part[p] + rng.uniform(-noise, noise, size=(B, len(idx), 3))
    # The bone of part p is joint 2p - joint 2p + 1.  The loss is discontinuous in the bone's direction at two kinds of pair: one
    # whose 'threshold' weight crosses `thr`, and one parallel to the bone, whose 'linear' / 'sin' weight reaches 0 so that the
    # pair leaves the count (in fp32 the cosine rounds to 1 from about 1 - 2e-7).  A part's joints are drawn again until no pair
    # of it comes within 2e-5 of the threshold or within 1e-5 of cosine 1 (parts too large for that table run without angles).
    kps = rng.normal(size=(B, 2 * P, 3)).astype(np.float32)
    for p, idx in enumerate(parts):
        if not 2 <= len(idx) <= angle_safe_max:
            continue
        iu = np.triu_indices(len(idx), 1)
        for b in range(B):
            g = x_gt[b, idx].astype(np.float64)
            d = (g[:, None, :] - g[None, :, :])[iu]
            d /= np.sqrt((d * d).sum(-1, keepdims=True))
            while True:
                bone = kps[b, 2 * p].astype(np.float64) - kps[b, 2 * p + 1].astype(np.float64)
                cos = np.minimum(np.abs(d @ bone) / np.sqrt(bone @ bone), 1.0)
                if (1.0 - cos).min() >= 1e-5 and np.abs(np.arccos(cos) * 2.0 / np.pi - thr).min() >= 2e-5:
                    break
                kps[b, 2 * p:2 * p + 2] = rng.normal(size=(2, 3)).astype(np.float32)
    return dict(parts=parts, x_gt=torch.from_numpy(x_gt), x_rec=torch.from_numpy(x_rec.astype(np.float32)), kps=torch.from_numpy(kps),
                skl_list=[[2 * p, 2 * p + 1] for p in range(P)], s_part=s_part)


def pairdist_scale(B, s_part, seed):
    """[B, P] factors on the ground-truth distances that keep every term's sign: 1 or 1.1 where the reconstruction shrinks
    (s = 0.95), 1 or 0.9 where it grows (s = 1.05)."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, 2, size=(B, len(s_part)))
    return torch.from_numpy(np.where(pick == 0, 1.0, np.where(np.asarray(s_part)[None, :] < 1, 1.1, 0.9)).astype(np.float32))


def pairdist_ref(x_rec, x_gt, kps, skl_list, parts, leaf, w_part, scale, w_mode, thr, relat, chunk=256):
    """The part pair-distance loss (csrc/part_loss.hip's header; oracle.ref_cpu.part_pairdist_loss) in float64, a block of rows
    at a time so that a part of several thousand vertices needs no [n, n, 3] tensor, with its analytic gradient w.r.t. x_rec
    -> dict(loss, grad [B, N1, 3], part_sum [P], part_cnt [P], thr_ambiguous, sign_ambiguous, zero_ambiguous, positive [P],
    negative [P]: the kept pairs of each part with e > 0 and with e < 0).
    thr_ambiguous: pairs i != j of a part with angle weights whose 'threshold' weight lies within 1e-5 of `thr`;
    sign_ambiguous: kept pairs with |e| < 1e-5 * w;
    zero_ambiguous: pairs i != j of a part with 'linear' or 'sin' weights whose cosine to the bone lies within 1e-6 of 1 - in fp32
    it rounds to 1 from about 1 - 2e-7, the weight becomes 0 and the pair leaves the count.
    The loss is discontinuous at all three; a comparison is meaningful only where every count is 0."""
    xr, xg, kp = (np.asarray(t, dtype=np.float64) for t in (x_rec, x_gt, kps))
    B, P = xr.shape[0], len(parts)
    sc = np.ones((B, P)) if scale is None else np.asarray(scale, dtype=np.float64)
    wp = np.asarray(w_part, dtype=np.float64)
    grad = np.zeros_like(xr)
    psum, pcnt, npos, nneg = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P)
    loss, amb_thr, amb_sign, amb_zero = 0.0, 0, 0, 0
    for p, idx in enumerate(parts):
        idx = np.asarray(idx, dtype=np.int64)
        n = len(idx)
        b_ = skl_list[p]
        bone = kp[:, b_[0]] - (kp[:, b_[1]] if len(b_) == 2 else (kp[:, b_[1]] + kp[:, b_[2]]) / 2)       # [B, 3]
        G, R = xg[:, idx], xr[:, idx]
        gp = np.zeros((B, n, 3))
        for i0 in range(0, n, chunk):
            # rows i0..i1 against the columns j > i only: (i, j) and (j, i) are both terms of the loss, and equal
            i1 = min(n, i0 + chunk)
            d = G[:, i0:i1, None, :] - G[:, None, i0:, :]
            dm = np.sqrt((d * d).sum(-1))
            off = (np.arange(i0, i1)[:, None] < np.arange(i0, n)[None, :])[None]
            if w_mode == "all_one" or p in leaf:
                w = np.ones_like(dm)
            else:
                km = np.sqrt((bone * bone).sum(-1))[:, None, None]
                with np.errstate(divide="ignore", invalid="ignore"):
                    cos = np.abs((d * bone[:, None, None, :]).sum(-1) / (dm * km))
                cos = np.clip(np.where(np.isnan(cos), 1.0, cos), 0.0, 1.0)
                if w_mode in ("linear", "sin"):
                    amb_zero += 2 * int((off & (cos > 1.0 - 1e-6)).sum())
                ang = np.arccos(cos) * 180.0 / np.pi
                w = ang / 90.0 if w_mode in ("linear", "threshold") else np.sin(ang / 180.0 * np.pi)
                if w_mode == "threshold":
                    amb_thr += 2 * int((off & (np.abs(w - thr) < 1e-5)).sum())
                    w = np.where(w < thr, 0.0, w)
            De = dm * sc[:, p][:, None, None]
            keep = off & ((w * De) != 0)
            u = R[:, i0:i1, None, :] - R[:, None, i0:, :]
            Dr = np.sqrt((u * u).sum(-1))
            De1 = np.where(keep, De, 1.0)
            e = w * Dr / De1 - w if relat else w * Dr - w * De
            amb_sign += 2 * int((keep & (np.abs(e) < 1e-5 * w)).sum())
            psum[p] += 2.0 * float(np.abs(e)[keep].sum())
            pcnt[p] += 2 * int(keep.sum())
            npos[p] += 2 * int((keep & (e > 0)).sum())
            nneg[p] += 2 * int((keep & (e < 0)).sum())
            live = keep & (Dr > 0)                                   # |.|' is undefined at Dr = 0: the pair adds nothing
            c = np.where(live, np.sign(e) * (w / De1 if relat else w) / np.where(Dr > 0, Dr, 1.0), 0.0)
            cu = c[..., None] * u
            gp[:, i0:i1] += cu.sum(2)                                # d term_ij / d r_i
            gp[:, i0:] -= cu.sum(1)                                  # d term_ij / d r_j
        if pcnt[p] > 0:
            loss += wp[p] * psum[p] / pcnt[p]
            grad[:, idx] = 2.0 * wp[p] / pcnt[p] * gp                # the sums above hold each unordered pair once
    return dict(loss=loss, grad=grad, part_sum=psum, part_cnt=pcnt, thr_ambiguous=amb_thr, sign_ambiguous=amb_sign, zero_ambiguous=amb_zero,
                positive=npos, negative=nneg)


# ---------------------------------------------------------------------------------------------- small kernels
def joint_l1_ref(x, target, J, keep):
    """mean |(J @ x[:, :N])[:, keep] - target| in float64 with autograd -> (kps [B, K, 3], loss, d loss / d x)."""
    xd = x.double().clone().requires_grad_(True)
    Jd = J.double()
    N = Jd.shape[1]
    kps = torch.matmul(Jd, xd[:, :N, :])
    loss = (kps[:, torch.as_tensor(keep, dtype=torch.long)] - target.double()).abs().mean()
    loss.backward()
    return kps.detach(), float(loss.detach()), xd.grad


def closed_mesh(nu, nv):
    """A closed triangle mesh of a torus grid with nu * nv vertices and 2 * nu * nv faces, consistently oriented
    -> (verts float64 [nu nv, 3], faces int32 [2 nu nv, 3])."""
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    verts = np.stack([(2 + 0.7 * np.cos(v)) * np.cos(u), (2 + 0.7 * np.cos(v)) * np.sin(u), 0.7 * np.sin(v)], -1).reshape(-1, 3)
    vid = lambda i, j: (i % nu) * nv + (j % nv)          # noqa: E731
    faces = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            faces += [[a, b, c], [a, c, d]]
    return verts, np.asarray(faces, dtype=np.int32)


def part_volume_ref(x_rec, x_gt, faces, fpi, parts):
    """(1/P) sum_p mean_b | |vr / vg| - 1 | with vol = sum over the part's faces of (a x b) . c, float64 with autograd
    -> (loss, d loss / d x_rec, vr [B, P], vg [B, P])."""
    xr = x_rec.double().clone().requires_grad_(True)
    xg = x_gt.double()
    f = torch.as_tensor(np.asarray(faces), dtype=torch.long)

    def signed(x):
        return (torch.linalg.cross(x[:, f[:, 0]], x[:, f[:, 1]], dim=2) * x[:, f[:, 2]]).sum(2)
    member = torch.as_tensor(np.asarray(fpi)[:, None] == np.asarray(parts)[None, :]).double()
    vr, vg = signed(xr) @ member, signed(xg) @ member
    loss = ((vr / vg).abs() - 1).abs().mean()
    loss.backward()
    return float(loss.detach()), xr.grad, vr.detach(), vg


def zpart_ref(z, measure, part_idx, measure_idx, relat):
    """mean | |z[:, part_idx]| / m[:, measure_idx] - 1 | (or | |z| - m |) in float64 with autograd -> (loss, d loss / d z, d)."""
    zd = z.double().clone().requires_grad_(True)
    zm = torch.sqrt((zd ** 2).sum(2))[:, torch.as_tensor(part_idx, dtype=torch.long)]
    mm = measure.double()[:, torch.as_tensor(measure_idx, dtype=torch.long)]
    d = zm / mm - 1 if relat else zm - mm
    loss = d.abs().mean()
    loss.backward()
    return float(loss.detach()), zd.grad, d.detach()
