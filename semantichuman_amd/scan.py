"""Fitting to unregistered point clouds: nearest-point search and the Chamfer loss (no reference counterpart).

  * `ScanBatch(clouds, device)`   ragged clouds -> one resident padded [B, Mmax, 3] tensor + counts (host packing, numpy)
  * `nearest(q, t, ...)`          -> sh_nearest_points: index and squared distance of each query's nearest target
  * `chamfer(x_hat, scans, ...)`  -> sh_nearest_points (one or both directions) + sh_chamfer_fwd / sh_chamfer_bwd, differentiable
                                     w.r.t. x_hat through the recorded indices

Distances are formed from coordinate differences in fp32 (include/sh_kernels.h states the expression), never from
|a|^2 + |b|^2 - 2ab, and no [B, N, M] matrix exists at any point.  Everything is deterministic.  Scans are expected in the
model's normalised frame: there is no rigid or similarity alignment here, no point-to-triangle distance and no file reader.
The search and the loss have no CPU path: tensors must live on the GPU.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops


def pack_clouds(clouds):
    """A list of [m_b, 3] arrays (or one [B, M, 3] array) -> (points float32 [B, Mmax, 3] zero-padded, counts int32 [B]).
    Host side, numpy only.  ValueError on an empty list, a wrong shape, NaN or inf."""
    if isinstance(clouds, np.ndarray) and clouds.ndim == 3:
        clouds = list(clouds)
    elif torch.is_tensor(clouds) and clouds.dim() == 3:
        clouds = list(clouds.detach().cpu().numpy())
    clouds = [c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c) for c in clouds]
    if len(clouds) == 0:
        raise ValueError("ScanBatch: no clouds")
    for b, c in enumerate(clouds):
        if c.ndim != 2 or c.shape[1] != 3:
            raise ValueError("ScanBatch: cloud %d has shape %s, expected [m, 3]" % (b, c.shape))
        if not np.isfinite(c).all():
            raise ValueError("ScanBatch: cloud %d holds NaN or inf" % b)
    counts = np.asarray([c.shape[0] for c in clouds], dtype=np.int32)
    pts = np.zeros((len(clouds), int(counts.max()), 3), dtype=np.float32)
    for b, c in enumerate(clouds):
        pts[b, :c.shape[0]] = c
    return pts, counts


class ScanBatch:
    """B point clouds resident on the device: `points` fp32 [B, Mmax, 3] (rows >= counts[b] are zero padding the kernels never
    read as points), `counts` int32 [B].  `host_counts` keeps the counts on the host."""

    def __init__(self, clouds, device):
        pts, counts = pack_clouds(clouds)
        dev = torch.device(device)
        self.host_counts = counts
        self.points = torch.from_numpy(pts).to(dev)
        self.counts = torch.from_numpy(counts).to(dev)

    def __len__(self):
        return self.points.shape[0]

    def select(self, sl):
        """The bodies `sl` (a slice) as a ScanBatch sharing this one's memory."""
        out = ScanBatch.__new__(ScanBatch)
        out.host_counts = self.host_counts[sl]
        out.points = self.points[sl]
        out.counts = self.counts[sl].contiguous()
        return out


def nearest(q, t, q_count=None, t_count=None, t_mask=None, chunks=0):
    """For every query q[b, j] its nearest target in t[b]: (idx int32 [B, nq], d2 fp32 [B, nq]), d2 the squared distance in the
    difference form of sh_kernels.h, idx the lowest index on an exact tie.  q_count / t_count [B]: live rows per body (None =
    all); t_mask [nt] or [B, nt]: False = target not allowed.  No allowed target: idx -1, d2 +inf; queries beyond q_count:
    idx -1, d2 0.  chunks: how many ranges the targets are split into (0 = chosen by the library; every split gives the same
    bits).  Not differentiable."""
    return ops.nearest_points(q.detach(), t.detach(), q_count, t_count, t_mask, chunks=chunks)


class _Chamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scans, n, v_mask, mask_sb, tau2, w_ms):
        s, cnt = scans.points, scans.counts
        rows = x.shape[1]
        idx_sm, d2_sm = ops.nearest_points(s, x, q_count=cnt, t_mask=v_mask, nt=n)
        idx_ms = d2_ms = None
        if w_ms > 0.0:
            idx_ms, d2_ms = ops.nearest_points(x, s, t_count=cnt)                   # all rows are queries: [B, rows] as the kernels index it
        loss, counts = ops.chamfer_fwd(d2_sm, cnt, d2_ms, rows, n, v_mask, mask_sb, tau2, w_ms)
        ctx.scans, ctx.n, ctx.v_mask, ctx.mask_sb, ctx.tau2, ctx.w_ms = scans, n, v_mask, mask_sb, tau2, w_ms
        ctx.save_for_backward(x, idx_sm, d2_sm, idx_ms, d2_ms, counts)
        return loss

    @staticmethod
    def backward(ctx, gL):
        x, idx_sm, d2_sm, idx_ms, d2_ms, counts = ctx.saved_tensors
        g = ops.chamfer_bwd(x, ctx.n, ctx.scans.points, ctx.scans.counts, idx_sm, d2_sm, idx_ms, d2_ms, ctx.v_mask, ctx.mask_sb, counts,
                            ctx.tau2, ctx.w_ms, gL.to(torch.float32).contiguous())
        return g, None, None, None, None, None, None


def chamfer(x_hat, scans, n=None, vertex_mask=None, trunc=None, w_model_to_scan=0.0):
    """Chamfer distance between decoded bodies and their scans, one value per body [B], differentiable w.r.t. x_hat:

        L[b] = mean_j min(|s_j - nn_x(s_j)|^2, trunc^2)  +  w_model_to_scan * mean_{i active} min(|x_i - nn_s(x_i)|^2, trunc^2)

    x_hat [B, rows, 3] fp32 on the GPU; scans: a ScanBatch (or clouds, packed on the spot) of the same B, in the model's
    normalised frame (no alignment is done here).  n: how many leading rows of x_hat are model vertices.  n=None means
    rows - 1, because every model of this package appends a dummy row to what it decodes; pass n=rows for a bare vertex tensor.
    Rows >= n are never matched and get no gradient - do not slice x_hat instead.  vertex_mask [n] or [B, n]: False = vertex
    takes no part (not a target, no term of its own).  trunc: distances beyond it are cut to it and stop pulling (None: none).
    w_model_to_scan = 0 skips the model -> scan search altogether - the setting for a partial scan.  The gradient flows through
    the nearest indices found in the forward pass; the scan takes none."""
    if not (torch.is_tensor(x_hat) and x_hat.is_cuda):
        raise RuntimeError("semantichuman_amd.scan.chamfer needs fp32 HIP vertices [B, rows, 3] (got %s); there is no CPU path"
                           % getattr(x_hat, "device", type(x_hat)))
    if not isinstance(scans, ScanBatch):
        scans = ScanBatch(scans, x_hat.device)
    B, rows, _ = ops._points(x_hat, "scan.chamfer")
    if len(scans) != B:
        raise ValueError("chamfer: %d bodies, %d scans" % (B, len(scans)))
    n = rows - 1 if n is None else int(n)
    if not 0 < n <= rows:
        raise ValueError("chamfer: n = %d outside (0, %d]" % (n, rows))
    w = float(w_model_to_scan)
    if not w >= 0.0:
        raise ValueError("chamfer: w_model_to_scan must be >= 0")
    if trunc is not None and not float(trunc) > 0.0:
        raise ValueError("chamfer: trunc must be > 0")
    tau2 = math.inf if trunc is None else float(trunc) ** 2
    v_mask, mask_sb = ops._mask_arg(vertex_mask, B, n, x_hat.device)
    return _Chamfer.apply(x_hat, scans, n, v_mask, mask_sb, tau2, w)
