"""Fitting to unregistered point clouds: nearest-point search and the Chamfer loss (no reference counterpart).

  * `ScanBatch(clouds, device)`   ragged clouds -> one resident padded [B, Mmax, 3] tensor + counts (host packing, numpy)
  * `nearest(q, t, ...)`          -> sh_nearest_points: index and squared distance of each query's nearest target
  * `FaceTable`, `nearest_surface(q, x, faces, ...)`, `closest_points(...)`  -> sh_nearest_surface: the exact closest point of the
                                     model's triangles to each scan point (face, squared distance, barycentric weights)
  * `chamfer(x_hat, scans, ...)`  -> sh_nearest_points (one or both directions) + sh_chamfer_fwd / sh_chamfer_bwd, differentiable
                                     w.r.t. x_hat through the recorded indices; with `faces=` the scan -> model term is measured
                                     to the surface (sh_nearest_surface, sh_chamfer_surface_bwd)
  * `Pose`, `moment_pose(...)`, `align(x, scans, ...)`  scan frame -> model frame: batched similarity ICP on the same matches
                                     (sh_transform_points, sh_align_moments, sh_align_solve); with `faces=` the scan -> model
                                     partner is the foot point on the surface (sh_nearest_surface, sh_align_moments_surface);
                                     with `step="plane"` the pose step is the linearised point-to-plane (Gauss-Newton) step along
                                     the model's normals (sh_align_plane_moments, sh_align_plane_solve) instead of the closed form
  * `ScanBatch(..., normals=)`, `vertex_normals(x, faces)`, `normal_angle=` on chamfer / align  matching by normal: the scan's
                                     normals and the model's area-weighted vertex normals (sh_vertex_normals) gate every pair of
                                     the vertex search (sh_nearest_points_gated) - off unless `normal_angle` is given
  * `estimate_normals(points, k)`, `ScanBatch(..., normals="estimate")`  normals of a bare cloud, from the cloud: per point the k
                                     nearest points of its own cloud and the direction of least spread among them
                                     (sh_cloud_normals) - unoriented unless `viewpoints` are given
  * `visible_vertices(x, faces, viewpoints)`, `visibility="viewpoint"` on chamfer / align  partial scans: the model vertices the
                                     sensor sees from `ScanBatch(..., viewpoints=)` - not occluded by any triangle, optionally
                                     facing the sensor (sh_vertex_visibility) - are the vertex mask of every search and term
  * `unproject_depth(depth, intrinsics, ...)`, `ScanBatch.from_depth(depth, intrinsics, device, ...)`  depth images as scans: the
                                     camera-frame point of every usable pixel, its normal from the pixel grid, oriented to the
                                     camera, and the rows packed in tile order (sh_depth_count, sh_depth_points)
  * `DepthField.from_depth(depth, intrinsics, ...)`, `free_space(x_hat, field, ...)`  what a depth image says about where the
                                     body is not: per pixel surface / empty / unknown and the nearest pixel that is not empty
                                     (sh_depth_field); per vertex a free-space and a silhouette term, differentiable
                                     (sh_free_space_fwd / _bwd) - off unless asked for
  * `unproject_depth_views(depth, intrinsics, extrinsics, ...)`, `ScanBatch.from_depth(..., extrinsics=)`  a rig of calibrated
                                     depth cameras as ONE scan per body in the rig's frame (sh_depth_views_count / _points);
                                     its `viewpoints` are [B, V, 3], and `visible_vertices` / `visibility="viewpoint"` then
                                     mean "seen by at least one camera" (sh_vertex_visibility_views, one sweep over the faces)
  * `views_overlap(scans, depth, intrinsics, extrinsics, tol=)`, `merge_views(scans, keep, seen)`, `merge_tol=` on the two
                                     above  the rows of a rig scan that a better-placed camera also measures, found by
                                     projection (sh_depth_views_overlap), and the batch without them (sh_scan_compact)
  * `DepthField.from_depth(..., extrinsics=)`, `free_space_cameras(field, pose)`, `free_space(x_hat, rig_field, pose=, cameras=)`
                                     the free-space and silhouette term for all cameras of a rig at once, the way from the
                                     model's frame into every camera's inside the kernels (sh_free_space_cameras,
                                     sh_free_space_views_fwd / _bwd)

Distances are formed from coordinate differences in fp32 (include/sh_kernels.h states the expression), never from
|a|^2 + |b|^2 - 2ab, and no [B, N, M] matrix exists at any point.  Everything is deterministic.  `chamfer` expects scans in the
model's normalised frame; `align` (and editing.register_scan, which alternates it with the fit) brings a scan there by a
translation, a rigid motion or a similarity.  The alignment works on vertex pairs, or with `faces=` on (scan point, foot point on
the surface) pairs - point-to-surface ICP in the same closed form (sh_align_moments_surface).  Depth images enter through
`ScanBatch.from_depth`, as arrays: there is still no file reader.  With `normal_angle` a pair is a match only when its two
normals agree to within that angle (a point with no compatible partner counts as truncated, so a gate needs `trunc`); the gate applies to vertex pairs, not to the surface distance of `faces=`.
The search, the loss and the alignment have no CPU path: tensors must live on the GPU.
"""
from __future__ import annotations

import math
import sys

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


def pack_normals(normals, counts, width):
    """Normals matching packed clouds row for row: a list of [m_b, 3] arrays (or one [B, M, 3] array) -> float32 [B, width, 3],
    every row normalised in float64 and rounded to fp32 once; a row of exact zeros stays zero ("unknown"), the padding is zero.
    ValueError on a shape that does not match the clouds, NaN or inf."""
    if isinstance(normals, np.ndarray) and normals.ndim == 3:
        normals = list(normals)
    elif torch.is_tensor(normals) and normals.dim() == 3:
        normals = list(normals.detach().cpu().numpy())
    normals = [c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c) for c in normals]
    if len(normals) != len(counts):
        raise ValueError("ScanBatch: %d clouds, normals for %d" % (len(counts), len(normals)))
    out = np.zeros((len(counts), int(width), 3), dtype=np.float32)
    for b, (c, m) in enumerate(zip(normals, counts)):
        if c.ndim != 2 or c.shape[1] != 3 or c.shape[0] != m:
            raise ValueError("ScanBatch: normals %d have shape %s, the cloud has [%d, 3]" % (b, c.shape, m))
        c = c.astype(np.float64)
        if not np.isfinite(c).all():
            raise ValueError("ScanBatch: normals %d hold NaN or inf" % b)
        big = np.abs(c).max(1, keepdims=True)                              # scaled first: no overflow or underflow in the squares
        c = c / np.where(big > 0, big, 1.0)
        out[b, :m] = c / np.where(big > 0, np.sqrt((c * c).sum(1, keepdims=True)), 1.0)
    return out


def _check_normal_k(what, k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not ops.CLOUD_K_MIN <= int(k) <= ops.CLOUD_K_MAX:
        raise ValueError("%s: the neighbour count must be an integer in [%d, %d], got %r" % (what, ops.CLOUD_K_MIN, ops.CLOUD_K_MAX, k))
    return int(k)


def pack_viewpoints(viewpoints, counts, width):
    """Sensor positions for `estimate_normals`, host side: [3] (one for all bodies) or [B, 3] (one per body) -> float32 [B, 3]; a
    list of [m_b, 3] arrays, one row per point (a fused multi-view scan), -> float32 [B, width, 3], zero-padded.  ValueError on
    a shape that fits none of the three, NaN or inf."""
    B = len(counts)
    v = viewpoints
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    if isinstance(v, (list, tuple)) and len(v) == B and all(np.ndim(c) == 2 for c in v):
        rows = [c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c) for c in v]
        out = np.zeros((B, int(width), 3), dtype=np.float32)
        for b, (c, m) in enumerate(zip(rows, counts)):
            if c.shape != (int(m), 3):
                raise ValueError("viewpoints: body %d has shape %s, its cloud has [%d, 3]" % (b, c.shape, m))
            out[b, :m] = c
    else:
        try:
            a = np.asarray(v, dtype=np.float32)
        except (ValueError, TypeError):
            a = None
        if a is not None and a.shape == (3,):
            out = np.broadcast_to(a, (B, 3)).copy()                                   # a copy: writable, and row-major for every B
        elif a is not None and a.shape == (B, 3):
            out = np.ascontiguousarray(a)
        else:
            raise ValueError("viewpoints must be [3], [%d, 3] or a list of %d arrays [m_b, 3], got %s"
                             % (B, B, "shape %s" % (a.shape,) if a is not None else type(viewpoints).__name__))
    if not np.isfinite(out).all():
        raise ValueError("viewpoints hold NaN or inf")
    return out


def morton_order(points, bits=10):
    """The permutation that sorts an [m, 3] cloud along the Morton (Z-order) curve of its own bounding box, `bits` bits per axis;
    a stable sort, so equal codes keep their order.  Host side, numpy only."""
    p = np.asarray(points, dtype=np.float64)
    if p.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    lo, hi = p.min(0), p.max(0)
    cell = np.where(hi > lo, hi - lo, 1.0)
    g = np.minimum(((p - lo) / cell * (1 << bits)).astype(np.int64), (1 << bits) - 1)
    code = np.zeros(p.shape[0], dtype=np.int64)
    for k in range(bits):
        for a in range(3):
            code |= ((g[:, a] >> k) & 1) << (3 * k + a)
    return np.argsort(code, kind="stable")


class ScanBatch:
    """B point clouds resident on the device: `points` fp32 [B, Mmax, 3] (rows >= counts[b] are zero padding the kernels never
    read as points), `counts` int32 [B].  `host_counts` keeps the counts on the host.

    order=None keeps every cloud's points in the order given.  order="morton" sorts each cloud along a space-filling curve at
    packing time (`morton_order`), so that points next to each other in memory are next to each other in space - what the
    surface search's cull lives on.  The permutation is kept on the host as `perm`, int64 [B, Mmax]: points[b, k] is the given
    cloud's point perm[b, k] (k < counts[b]; -1 in the padding); `perm` is None when nothing was sorted.  A Chamfer value does
    not depend on the order beyond the rounding of its sum.

    normals: None, or the clouds' normals row for row (a list of [m_b, 3] arrays or one [B, M, 3] array; `pack_normals`): kept as
    `normals`, fp32 [B, Mmax, 3] unit rows on the device, sorted with their points; a zero row means "unknown".  They are used
    only where a `normal_angle` is asked for.

    normals="estimate": the clouds carry none - a depth camera's output, a fused cloud - and they are estimated from the resident
    points, after any sort, by `estimate_normals(self, normal_k, viewpoints)` (sh_cloud_normals: the direction of least spread of
    each point's normal_k nearest points, the point included) and kept as `normals` exactly as given ones are: fp32 unit rows, a
    zero row where the neighbourhood is coincident or collinear.  viewpoints: None, or where the sensor stood, in the clouds'
    frame - [3], [B, 3] or a list of [m_b, 3] arrays (one row per point, in the order of the clouds given; sorted with them) - and
    every normal then points into its viewpoint's half space.  Without viewpoints the normals are UNORIENTED: the sign is a
    convention (largest component positive), so about half of them point into the body, and a gate narrower than 90 degrees
    rejects correct partners; a gate blind to orientation (on |cos|) is not part of the library.
    normal_k is read only with normals="estimate".  ValueError for a normal_k outside [3, 64] or viewpoints of another shape.

    `viewpoints`: fp32 [B, 3] on the device when a per-body viewpoint ([3] or [B, 3]) was given, with or without
    normals="estimate" - what `visibility="viewpoint"` of chamfer / align reads; None otherwise (per-point viewpoints serve the
    normals' orientation only).  A row set to NaN afterwards marks a body as a full scan: no viewpoint, every vertex visible.
    Without normals="estimate" a viewpoint that cannot be packed (another shape, NaN or inf) raises nothing here, as ever; the
    field is None and `visibility="viewpoint"` later names the reason.

    `pixels`: int32 [B, Mmax] on a batch made by `from_depth` - the pixel v * W + u each row came from, -1 in the padding; None on
    batches made any other way.

    A RIG batch - a scan fused from V sensors - carries `viewpoints` fp32 [B, V, 3] instead: the camera centres, a NaN row for an
    absent camera; `visibility="viewpoint"` then means "seen by at least one of them" (sh_vertex_visibility_views).
    `from_depth(..., extrinsics=)` makes one, with `view` uint8 [B, Mmax] (the camera each row came from, 255 in the padding) and
    `view_first` int32 [B, V + 1]; rig_viewpoints=[V, 3] or [B, V, 3] (at most 32 views, NaN rows allowed, no inf) sets the
    field for a cloud fused elsewhere and takes the place of a per-body `viewpoints` there (per-point viewpoints still orient
    estimated normals).  `seen`: None, or on a batch made by `merge_views` / `from_depth(..., merge_tol=)` int32 [B, Mmax] read as
    unsigned - bit c set where camera c also measured the row's surface point (`views_overlap`), 0 in the padding."""

    viewpoints = None                                                                   # for batches made without __init__ or _from_parts
    viewpoints_error = None
    pixels = None
    view = None
    view_first = None
    seen = None

    def __init__(self, clouds, device, order=None, normals=None, normal_k=16, viewpoints=None, rig_viewpoints=None):
        if order not in (None, "morton"):
            raise ValueError("ScanBatch: order must be None or 'morton'")
        estimate = isinstance(normals, str)
        if estimate:
            if normals != "estimate":
                raise ValueError("ScanBatch: normals must be None, arrays or 'estimate', got %r" % (normals,))
            normal_k = _check_normal_k("ScanBatch: normal_k", normal_k)
        pts, counts = pack_clouds(clouds)
        if torch.is_tensor(rig_viewpoints):
            rig_viewpoints = rig_viewpoints.detach().cpu()
        rig = None if rig_viewpoints is None else _view_arg("ScanBatch: rig_viewpoints", rig_viewpoints, len(counts), None, rig=True)
        view = None
        if viewpoints is not None:
            try:
                view = pack_viewpoints(viewpoints, counts, pts.shape[1])
            except ValueError:
                if estimate:
                    raise
                view = None                                                    # without "estimate" a viewpoint that fits no shape is not read, as ever
                self.viewpoints_error = str(sys.exc_info()[1])
        nrm = None if normals is None or estimate else pack_normals(normals, counts, pts.shape[1])
        self.perm = None
        if order == "morton":
            self.perm = np.full(pts.shape[:2], -1, dtype=np.int64)
            for b, m in enumerate(counts):
                self.perm[b, :m] = morton_order(pts[b, :m])
                pts[b, :m] = pts[b, :m][self.perm[b, :m]]
                if nrm is not None:
                    nrm[b, :m] = nrm[b, :m][self.perm[b, :m]]
                if view is not None and view.ndim == 3:
                    view[b, :m] = view[b, :m][self.perm[b, :m]]
        dev = torch.device(device)
        self.host_counts = counts
        self.points = torch.from_numpy(pts).to(dev)
        self.counts = torch.from_numpy(counts).to(dev)
        self.normals = None if nrm is None else torch.from_numpy(nrm).to(dev)
        view = None if view is None else torch.from_numpy(view).to(dev)
        self.viewpoints = rig.to(dev) if rig is not None else view if view is not None and view.dim() == 2 else None
        if estimate:
            self.normals = ops.cloud_normals(self.points, self.counts, normal_k, view)[0]

    def __len__(self):
        return self.points.shape[0]

    @classmethod
    def _from_parts(cls, points, counts, host_counts, perm, normals, viewpoints=None, pixels=None, view=None, view_first=None, seen=None):
        """A ScanBatch around tensors that are already packed and resident: every field, nothing copied or checked."""
        out = cls.__new__(cls)
        out.points, out.counts, out.host_counts, out.perm, out.normals = points, counts, host_counts, perm, normals
        out.viewpoints, out.pixels, out.view, out.view_first, out.seen = viewpoints, pixels, view, view_first, seen
        return out

    @classmethod
    def from_depth(cls, depth, intrinsics, device, extrinsics=None, merge_tol=None, **options):
        """Depth images as a batch of scans: `unproject_depth(depth, intrinsics, device=device, **options)` kept whole - points in
        the camera's frame in tile order (perm None), counts, the grid normals (oriented to the camera; a zero row: unknown),
        `viewpoints` = zeros [B, 3] (the camera centre) and `pixels`.  Ready for normal_angle=, gate_on=, visibility="viewpoint"
        and robust= without further arguments.  One host synchronisation, to read the counts.
        extrinsics: None, or the camera -> rig transforms of a rig of V depth cameras - then `unproject_depth_views(depth,
        intrinsics, extrinsics, device=device, **options)` kept whole as a rig batch: one fused scan per body in the rig's frame,
        view-major, with `pixels`, `view`, `view_first` and `viewpoints` fp32 [B, V, 3] = the camera centres t (NaN for an absent
        camera).  Still one host synchronisation.
        merge_tol: None, or - a rig only - a depth tolerance >= 0: the rows that a better-placed camera also measures within it are
        dropped before the batch is made, `merge_views(scans, *views_overlap(scans, ..., tol=merge_tol))` on the batch described
        above with the images still resident, and `seen` is kept.  That costs TWO host synchronisations instead of one: the kept
        counts are read as well.  ValueError for a merge_tol without extrinsics, negative or NaN.
        distortion= (among the options): the lens, as in `unproject_depth` / `unproject_depth_views`; it works together with
        merge_tol.  A ready `CameraRays` launches nothing more than the default path does."""
        if extrinsics is not None:
            rows = _unproject_depth_views(depth, intrinsics, extrinsics, device=device, merge_tol=merge_tol, **options)
            points, normals, pixel, view, view_first, counts, host_counts, ext = rows[:8]
            return cls._from_parts(points, counts, host_counts, None, normals, viewpoints=torch.from_numpy(ext[:, :, 9:].copy()).to(points.device),
                                   pixels=pixel, view=view, view_first=view_first, seen=rows[8] if len(rows) > 8 else None)
        if merge_tol is not None:
            raise ValueError("ScanBatch.from_depth: merge_tol needs a rig (extrinsics=); one camera has no overlap")
        points, normals, pixel, counts, host_counts = _depth_rows("unproject_depth", depth, intrinsics, device=device, **options)
        return cls._from_parts(points, counts, host_counts, None, normals,
                               viewpoints=torch.zeros((points.shape[0], 3), dtype=torch.float32, device=points.device), pixels=pixel)

    def select(self, sl):
        """The bodies `sl` (a slice) as a ScanBatch sharing this one's memory."""
        return ScanBatch._from_parts(self.points[sl], self.counts[sl].contiguous(), self.host_counts[sl],
                                     None if self.perm is None else self.perm[sl], None if self.normals is None else self.normals[sl],
                                     viewpoints=None if self.viewpoints is None else self.viewpoints[sl].contiguous(),
                                     pixels=None if self.pixels is None else self.pixels[sl], view=None if self.view is None else self.view[sl],
                                     view_first=None if self.view_first is None else self.view_first[sl],
                                     seen=None if self.seen is None else self.seen[sl])


def estimate_normals(points_or_scans, k=16, viewpoints=None, counts=None):
    """Normals of bare point clouds, estimated from the clouds themselves (sh_cloud_normals; include/sh_kernels.h, "Cloud
    normals").  points_or_scans: a ScanBatch, or fp32 HIP points [B, M, 3] with optional live counts [B].  For every point: its
    neighbourhood is the k nearest points of its own cloud, itself included and every tie at the k-th distance with them (k is
    cut to the cloud's size); the normal is the eigenvector of the smallest eigenvalue of the neighbourhood's covariance (fp64
    moments of fp32 differences, a fixed-sweep Jacobi), a unit fp32 row.  -> (normals fp32 [B, M, 3], variation fp32 [B, M] =
    l0 / (l0 + l1 + l2), 0 on a plane and large on edges and noise, radius2 fp32 [B, M] the squared k-th distance, count int32
    [B, M] the neighbourhood's size), on the device; rows beyond a cloud's count are zero in all four.  A point whose
    neighbourhood is coincident or collinear, or has fewer than 3 members, gets the zero normal: "unknown", as everywhere.

    viewpoints: None - the sign is then a convention (the component of largest magnitude is positive) and the normals are
    UNORIENTED - or the sensor positions: host [3] / [B, 3] / a list of [m_b, 3] arrays (`pack_viewpoints`), or an fp32 HIP
    tensor [B, 3] / [B, M, 3], rows in the order of the points as they are resident.  A normal is then flipped when it points
    away from its viewpoint.  Brute force, O(M^2) per cloud: meant to run once per scan.  Deterministic - the same bits for a
    cloud alone and inside any padded batch.  Not differentiable.  ValueError for k outside [3, 64]."""
    k = _check_normal_k("estimate_normals: k", k)
    if isinstance(points_or_scans, ScanBatch):
        if counts is not None:
            raise ValueError("estimate_normals: a ScanBatch brings its own counts")
        pts, cnt, host_counts = points_or_scans.points, points_or_scans.counts, points_or_scans.host_counts
    else:
        pts = points_or_scans.detach() if torch.is_tensor(points_or_scans) else points_or_scans
        B, M, _ = ops._points(pts, "scan.estimate_normals")
        cnt = ops._count_arg(counts, B, pts.device)
        host_counts = None
    view = viewpoints
    if view is not None and not (torch.is_tensor(view) and view.is_cuda):
        if host_counts is None:
            host_counts = np.full(pts.shape[0], pts.shape[1], np.int64) if cnt is None else cnt.cpu().numpy()
        view = torch.from_numpy(pack_viewpoints(view, host_counts, pts.shape[1])).to(pts.device)
    elif view is not None:
        view = view.detach().to(torch.float32).contiguous()
    return ops.cloud_normals(pts, cnt, k, view)


def _intrinsics_arg(what, intrinsics, shapes):
    """(fx, fy, cx, cy) rows as a float64 array whose shape is one of `shapes`, else ValueError."""
    try:
        k = np.asarray(intrinsics.detach().cpu().numpy() if torch.is_tensor(intrinsics) else intrinsics, dtype=np.float64)
    except (ValueError, TypeError):
        k = None
    if k is None or k.shape not in shapes:
        raise ValueError("%s: intrinsics must be (fx, fy, cx, cy) as %s or %s, got %s"
                         % (what, ", ".join(str(list(s)) for s in shapes[:-1]), list(shapes[-1]),
                            "shape %s" % (k.shape,) if k is not None else type(intrinsics).__name__))
    return k


# ------------------------------------------------------------------------------------------------ lens distortion
def _distortion_arg(what, distortion, leads):
    """OpenCV coefficients (k1, k2, p1, p2[, k3[, k4, k5, k6]]) - 4, 5 or 8 per camera, with a leading shape among `leads` - as a
    float32 array lead + (8,), shorter sets zero-padded in OpenCV's order; else ValueError."""
    try:
        c = np.asarray(distortion.detach().cpu().numpy() if torch.is_tensor(distortion) else distortion, dtype=np.float64)
    except (ValueError, TypeError):
        c = None
    if c is None or c.ndim < 1 or c.shape[-1] not in (4, 5, 8):
        raise ValueError("%s: distortion must hold 4, 5 or 8 coefficients per camera (k1, k2, p1, p2, k3, k4, k5, k6), got %s"
                         % (what, "shape %s" % (c.shape,) if c is not None else type(distortion).__name__))
    if c.shape[:-1] not in leads:
        raise ValueError("%s: distortion of shape %s does not match the cameras: its leading shape must be one of %s"
                         % (what, c.shape, ", ".join(str(list(l)) for l in leads)))
    if not np.isfinite(c).all():
        raise ValueError("%s: distortion coefficients must be finite" % what)
    out = np.zeros(c.shape[:-1] + (8,), np.float32)
    out[..., :c.shape[-1]] = c
    return out


class CameraRays:
    """A calibrated camera's lens, resident on the device (sh_camera_rays; include/sh_kernels.h, "Camera rays"): `rays` fp32
    lead + [H, W, 2], every pixel's ray (x, y) - the pixel sees along (x, y, 1) -, (NaN, NaN) where the model cannot be inverted;
    `limit` fp32 lead, the largest x^2 + y^2 the forward model is trusted to (beyond it a point is outside the image: the model
    may fold back); `coeffs` fp32 lead + [8] in OpenCV's order, `intrinsics` fp32 lead + [4]; `complete` (a host bool): every
    pixel of every camera has a ray; `shape` = (H, W).  lead is (), [V] or [B, V] ([B] for one camera per body).  Made by
    `camera_rays`; what distortion= takes for a fixed camera over many calls."""

    def __init__(self, rays, limit, coeffs, intrinsics, complete, host):
        self.rays, self.limit, self.coeffs, self.intrinsics, self.complete = rays, limit, coeffs, intrinsics, bool(complete)
        self.shape = tuple(rays.shape[-3:-1])
        self._host = host                                                   # (intrinsics, coefficients) float32 numpy, as uploaded

    @property
    def lead(self):
        return tuple(self.limit.shape)

    def select(self, sl):
        """The bodies `sl` (a slice) of tables with a batch axis, sharing memory."""
        return CameraRays(self.rays[sl], self.limit[sl], self.coeffs[sl], self.intrinsics[sl], self.complete, tuple(h[sl] for h in self._host))

    def _planes(self, lead):
        """(table, coefficients, limit) as contiguous tensors of leading shape `lead` (the same number of cameras)."""
        H, W = self.shape
        return (self.rays.reshape(lead + (H, W, 2)).contiguous(), self.coeffs.reshape(lead + (8,)).contiguous(), self.limit.reshape(lead).contiguous())


def camera_rays(intrinsics, distortion, shape, device=None):
    """The lens of calibrated depth cameras as ray tables -> `CameraRays` (sh_camera_rays; include/sh_kernels.h, "Camera rays").
    intrinsics: (fx, fy, cx, cy) as [4], [V, 4] or [B, V, 4]; distortion: OpenCV's rational model (k1, k2, p1, p2, k3, k4, k5, k6),
    4, 5 or 8 coefficients per camera (shorter sets are zero-padded in that order) as [k], [V, k] or [B, V, k]; the two leading
    shapes broadcast.  shape = (H, W); device: None is the default HIP device.  Per pixel centre the model is inverted by 20
    fixed-point steps in fp64 and checked by one forward evaluation: a pixel whose reprojection misses by more than 1e-3 pixel
    has no ray (NaN) - the wrappers that take the result then mask it.  Two launches per call and ONE host synchronisation, to
    read `complete`.  Deterministic: the same bits for a camera alone and among others.  ValueError (before the device is used)
    for a wrong coefficient count, shapes that do not broadcast, non-finite values or fx / fy that are not positive."""
    what = "camera_rays"
    try:
        H, W = (int(v) for v in shape)
    except (ValueError, TypeError):
        H = W = -1
    if H < 1 or W < 1:
        raise ValueError("%s: shape must be (H, W) with both at least 1, got %r" % (what, shape))
    try:
        k = np.asarray(intrinsics.detach().cpu().numpy() if torch.is_tensor(intrinsics) else intrinsics, dtype=np.float64)
    except (ValueError, TypeError):
        k = None
    if k is None or k.ndim not in (1, 2, 3) or k.shape[-1] != 4:
        raise ValueError("%s: intrinsics must be (fx, fy, cx, cy) as [4], [V, 4] or [B, V, 4]" % what)
    if not np.isfinite(k).all() or not (k[..., :2] > 0).all():
        raise ValueError("%s: fx and fy must be finite and positive, cx and cy finite" % what)
    n = np.shape(distortion.detach().cpu().numpy() if torch.is_tensor(distortion) else distortion)
    try:
        lead = np.broadcast_shapes(k.shape[:-1], tuple(n[:-1]))
    except ValueError:
        raise ValueError("%s: distortion of shape %s does not match the cameras: intrinsics of shape %s" % (what, tuple(n), k.shape)) from None
    if len(lead) > 2:
        raise ValueError("%s: distortion of shape %s does not match the cameras: at most [B, V, k]" % (what, tuple(n)))
    c = _distortion_arg(what, distortion, (tuple(n[:-1]),))
    return _camera_rays(np.broadcast_to(k.astype(np.float32), lead + (4,)).copy(), np.broadcast_to(c, lead + (8,)).copy(), H, W, device)


def _camera_rays(k, c, H, W, device):
    """`camera_rays` on checked float32 arrays lead + (4,) and lead + (8,)."""
    lead = k.shape[:-1]
    k, c = np.array(k, np.float32), np.array(c, np.float32)                            # own, writable copies: they are kept
    dev = torch.device(device if device is not None else "cuda")
    kd, cd = torch.from_numpy(k.reshape(-1, 4)).to(dev), torch.from_numpy(c.reshape(-1, 8)).to(dev)
    rays, limit, complete = ops.camera_rays(kd, cd, H, W)
    return CameraRays(rays.view(lead + (H, W, 2)), limit.view(lead), cd.view(lead + (8,)), kd.view(lead + (4,)),
                      bool(complete.min().item()) if complete.numel() else True, (k, c))          # the one synchronisation


def _calibration(what, distortion, k, B, V, H, W, device):
    """distortion= of the depth wrappers -> None, or (CameraRays, lead): the cameras of B bodies of V views each (V = 0: one
    camera per body) whose intrinsics are k float32 [B * max(V, 1), 4]; lead is the leading shape ops takes - [1] / [V] when one
    table per camera serves every body, [B] / [B, V] otherwise.  Coefficients: a table per camera when neither they nor the
    intrinsics differ between the bodies, else per body.  A ready CameraRays must fit: ValueError for another image size,
    camera count or intrinsics.  Nothing is launched for a ready one; for coefficients the device is used only after the checks."""
    if distortion is None:
        return None
    per = max(V, 1)
    shared, own = ((V,) if V else (1,)), ((B, V) if V else (B,))
    kk = k.reshape(B, per, 4)
    if isinstance(distortion, CameraRays):
        cr = distortion
        if cr.shape != (H, W):
            raise ValueError("%s: the CameraRays is of %d x %d images, the depth of %d x %d" % ((what,) + cr.shape + (H, W)))
        if cr.lead == shared or (per == 1 and cr.lead == ()):
            lead = shared
        elif cr.lead == own:
            lead = own
        else:
            raise ValueError("%s: the CameraRays holds cameras %s, the images need %s or %s" % (what, list(cr.lead), list(shared), list(own)))
        if not np.array_equal(np.broadcast_to(cr._host[0].reshape(-1, per, 4), (B, per, 4)), kk):
            raise ValueError("%s: the CameraRays was made for other intrinsics" % what)
        return cr, lead
    c = _distortion_arg(what, distortion, ((), (V,), (B, V)) if V else ((), (B,)))
    c = np.broadcast_to(c[:, None] if V == 0 and c.ndim == 2 else c, (B, per, 8))
    if (kk == kk[:1]).all() and (c == c[:1]).all():
        return _camera_rays(np.ascontiguousarray(kk[0].reshape(shared + (4,))), np.ascontiguousarray(c[0].reshape(shared + (8,))), H, W, device), shared
    return _camera_rays(np.ascontiguousarray(kk.reshape(own + (4,))), np.ascontiguousarray(c.reshape(own + (8,))), H, W, device), own


def _ray_mask(cal, m, B, V, H, W):
    """The mask rule: with an incomplete table "this pixel has a ray" is ANDed into the mask m (uint8 [B * max(V, 1), H, W] or None)
    with torch ops before the validity rules run in the kernels, which never test a ray."""
    cr, lead = cal
    if cr.complete:
        return m
    per = max(V, 1)
    has = ~torch.isnan(cr.rays.reshape(-1, per, H, W, 2)[..., 0])                        # [1 or B, per, H, W]
    has = has.expand(B, per, H, W).reshape(B * per, H, W).to(torch.uint8)
    return has.contiguous() if m is None else (m & has).contiguous()


def _depth_inputs(what, depth, intrinsics, mask, z_range):
    """The checks `unproject_depth` and `DepthField.from_depth` share, nothing moved to the device yet -> (depth [B, H, W] fp32 or
    int16 words, intrinsics float32 numpy [B, 4], mask [B, H, W] or None, near, far)."""
    if torch.is_tensor(depth):
        d = depth.detach()
        if hasattr(torch, "uint16") and d.dtype == torch.uint16:
            d = d.view(torch.int16)                                                     # the words as they are: the kernel reads them unsigned
        known = d.dtype in (torch.float32, torch.int16)
    else:
        d = np.asarray(depth)
        known = d.dtype in (np.float32, np.uint16)
        if known:
            d = np.ascontiguousarray(d)
            d = torch.from_numpy(d.view(np.int16) if d.dtype == np.uint16 else d)
    if not known or d.dim() not in (2, 3) or min(d.shape) < 1:
        raise ValueError("%s: depth must be fp32 or 16-bit unsigned, [H, W] or [B, H, W] and not empty, got %s %s"
                         % (what, getattr(depth, "dtype", type(depth).__name__), tuple(getattr(depth, "shape", ()))))
    lead = () if d.dim() == 2 else (d.shape[0],)
    d = d.reshape((-1,) + tuple(d.shape[-2:]))
    B = d.shape[0]
    k = np.broadcast_to(_intrinsics_arg(what, intrinsics, ((4,), (B, 4))).astype(np.float32), (B, 4)).copy()
    if not np.isfinite(k).all() or not (k[:, :2] > 0).all():
        raise ValueError("%s: fx and fy must be finite and positive, cx and cy finite" % what)
    m = mask
    if m is not None:
        m = m.detach() if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m))
        if tuple(m.shape) != lead + tuple(d.shape[-2:]) or m.is_floating_point() or m.is_complex():
            raise ValueError("%s: mask must be a bool or integer array of the depth's shape %s, got %s %s"
                             % (what, lead + tuple(d.shape[-2:]), m.dtype, tuple(m.shape)))
        m = m.reshape(d.shape)
    near, far = -math.inf, math.inf
    if z_range is not None:
        try:
            near, far = (float(v) for v in z_range)
        except (ValueError, TypeError):
            near = math.nan
        if not near <= far:
            raise ValueError("%s: z_range must be a pair (near, far) with near <= far, got %r" % (what, z_range))
    return d, k, m, near, far


def _depth_upload(d, k, m, device):
    """What `_depth_inputs` returned, resident: (depth, intrinsics fp32 [B, 4], mask uint8 or None) on `device` (None: the
    depth's, or the default HIP device for a host array)."""
    dev = torch.device(device if device is not None else d.device if d.is_cuda else "cuda")
    return d.to(dev).contiguous(), torch.from_numpy(k).to(dev), None if m is None else (m.to(dev) != 0).to(torch.uint8).contiguous()


def _depth_rows(what, depth, intrinsics, ext=None, depth_scale=1.0, mask=None, z_range=None, max_step=None, drop_isolated=False, stride=1,
                device=None, merge_tol=None, distortion=None):
    """`unproject_depth` (ext None), with the counts as the host read them as a fifth result - and what `unproject_depth_views`
    shares with it: `_depth_inputs` and the checks of max_step and stride - every ValueError before the device is used -, then
    upload, count, read the counts once, points.  ext: a rig's float32 [B, V, 12] - depth, intrinsics and mask then hold an image
    per row, body-major, and ops.depth_views_points' results come first.  merge_tol (a rig only, checked by the caller): the rows
    are merged with the resident images (`_merge_rows`: a second synchronisation) and `seen` is an eighth result.  distortion: None
    - the launches and bits of ever -, or the lens (`_calibration`): the "Camera rays" forms of the same launches."""
    d, k, m, near, far = _depth_inputs(what, depth, intrinsics, mask, z_range)
    step = math.inf if max_step is None else float(max_step)
    if not step >= 0:
        raise ValueError("%s: max_step must be None or >= 0, got %r" % (what, max_step))
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 1:
        raise ValueError("%s: stride must be an integer >= 1, got %r" % (what, stride))
    B, V = (d.shape[0], 0) if ext is None else tuple(ext.shape[:2])
    dev = device if device is not None or not d.is_cuda else d.device
    cal = _calibration(what, distortion, k, B, V, d.shape[-2], d.shape[-1], dev)
    d, k, m = _depth_upload(d, k, m, device)
    rays = {}
    if cal is not None:
        m = _ray_mask(cal, m, B, V, d.shape[-2], d.shape[-1])
        rays = dict(rays=cal[0]._planes(cal[1]))
    lead, count, points = (d, k), ops.depth_count, ops.depth_points
    if ext is not None:
        rig = tuple(ext.shape[:2])
        lead = (d.view(rig + tuple(d.shape[-2:])), k.view(rig + (4,)), torch.from_numpy(ext).to(d.device))
        m = None if m is None else m.view(lead[0].shape)
        count, points = ops.depth_views_count, ops.depth_views_points
    opts = dict(mask=m, depth_scale=depth_scale, z_near=near, z_far=far, max_step=step, drop_isolated=drop_isolated, stride=int(stride), **rays)
    counts, ws = count(*lead, **opts)
    host_counts = counts.cpu().numpy()                                                  # the one synchronisation
    most = int(host_counts.max())
    rows = points(*lead, counts, ws, max(most, 1), most, **opts)
    if merge_tol is None:
        return rows + (counts, host_counts)
    seen, keep = ops.depth_views_overlap(*lead, rows[0], rows[1], rows[3], counts, merge_tol, mask=m, depth_scale=depth_scale, z_near=near, z_far=far,
                                         **rays)
    return _merge_rows(rows[0], rows[1], rows[2], rows[3], counts, rig[1], keep, seen)


def unproject_depth(depth, intrinsics, *, depth_scale=1.0, mask=None, z_range=None, max_step=None, drop_isolated=False, stride=1, device=None,
                    distortion=None):
    """Depth images -> scans (sh_depth_count, sh_depth_points; include/sh_kernels.h, "Depth images").  depth: a host array or a
    tensor [B, H, W] or [H, W], fp32 or 16-bit unsigned words (a tensor of int16 is read as such words); z = raw * depth_scale.
    intrinsics: (fx, fy, cx, cy) as [4] or [B, 4]; without distortion= an ideal pinhole.  A pixel is valid when z is finite and positive, lies
    in z_range = (near, far) if given, is not the word 0, and mask (bool or integer, the depth's shape) is non-zero there.  Its
    point is ((u - cx) z / fx, (v - cy) z / fy, z) in the camera's frame.  Its normal comes from its grid neighbours - central
    differences where both are usable, one-sided where one is; a neighbour is usable when valid and within max_step in depth
    (None: any step), so no tangent crosses a silhouette - as the unit cross product in fp64, turned towards the camera; a zero
    row where a tangent is missing: "unknown", as everywhere.  Kept: valid pixels on the grid of every stride-th column and row
    (normals still read the full-resolution neighbours) and, with drop_isolated, of known normal - which drops flying pixels
    that max_step has cut off on all sides.
    -> (points fp32 [B, M, 3], normals fp32 [B, M, 3], pixel int32 [B, M] = v * W + u, counts int32 [B]) on `device` (None: the
    depth's, or the default HIP device for a host array), M the largest count (at least 1); rows beyond a count are zeros, zeros
    and -1.  Rows are in 16 x 16 tile order, Z-order inside a tile: neighbours in memory are neighbours on the surface.  One host
    synchronisation, to read the counts: a packing-time operation.  Deterministic - the same bits for an image alone and inside
    any batch.  Not differentiable.  ValueError for wrong shapes or dtypes, fx / fy not finite and positive, stride < 1 or a
    negative max_step.
    distortion: None - the launches and bits described above -, or the camera's lens (include/sh_kernels.h, "Camera rays"): OpenCV
    coefficients (k1, k2, p1, p2, k3, k4, k5, k6), 4, 5 or 8 of them as [k] or [B, k], or a ready `CameraRays` (`camera_rays`) -
    the form for a fixed camera over many calls, no ray launch then; coefficients cost the two launches and the synchronisation
    of `camera_rays` per call.  A pixel's point is then (x z, y z, z) with (x, y) its ray from the table, and its neighbours'
    points come from theirs (sh_depth_rays_count / _points); everything else is as above.  A pixel the lens model cannot be
    inverted at has no ray and counts as masked.  All-zero coefficients take this path too and agree with the pinhole result to
    rounding, not bit for bit: x z against ((u - cx) z) / fx.  ValueError (before the device is used) for a wrong coefficient
    count, a shape that does not match the cameras, non-finite coefficients, or a CameraRays of another image size, camera count
    or intrinsics."""
    return _depth_rows("unproject_depth", depth, intrinsics, None, depth_scale, mask, z_range, max_step, drop_isolated, stride, device,
                       distortion=distortion)[:4]


def pack_extrinsics(extrinsics, what="extrinsics"):
    """Camera -> rig transforms, host side: [V, 3, 4] or [B, V, 3, 4] = (R | t), or 4 x 4 matrices whose last row is 0 0 0 1 ->
    (float32 [B, V, 12] in the layout of sh_transform_points - R row-major, then t -, batched: whether a batch axis was given).
    An all-NaN matrix is an absent camera and is kept as NaN.  ValueError on any other shape, a matrix that mixes NaN with
    numbers or holds inf, a last row that is not 0 0 0 1, or a rotation block with max |R^T R - I| > 1e-4 or det <= 0."""
    e = extrinsics.detach().cpu().numpy() if torch.is_tensor(extrinsics) else extrinsics
    try:
        e = np.asarray(e, dtype=np.float64)
    except (ValueError, TypeError):
        e = None
    if e is None or e.ndim not in (3, 4) or e.shape[-2:] not in ((3, 4), (4, 4)) or min(e.shape) < 1:
        raise ValueError("%s: must be [V, 3, 4] or [B, V, 3, 4] (or 4 x 4 matrices), got %s"
                         % (what, "shape %s" % (e.shape,) if e is not None else type(extrinsics).__name__))
    batched = e.ndim == 4
    e = e.reshape((-1,) + e.shape[-3:]) if batched else e[None]
    absent = np.isnan(e).all((-2, -1))
    if not np.isfinite(e[~absent]).all():
        raise ValueError("%s: a matrix holds NaN or inf (an absent camera is a matrix of NaN only)" % what)
    if e.shape[-2] == 4:
        if not (e[~absent][:, 3] == np.array([0.0, 0.0, 0.0, 1.0])).all():
            raise ValueError("%s: the last row of a 4 x 4 matrix must be 0 0 0 1" % what)
        e = e[..., :3, :]
    R = e[~absent][:, :, :3]
    if R.size and (np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() > 1e-4 or (np.linalg.det(R) <= 0).any()):
        raise ValueError("%s: every rotation block must be a proper rotation (max |R^T R - I| <= 1e-4, det > 0; no scale, no mirror)" % what)
    out = np.concatenate([e[..., :3].reshape(e.shape[:2] + (9,)), e[..., 3]], -1).astype(np.float32)
    return np.ascontiguousarray(out), batched


def _check_merge_tol(what, tol, name="merge_tol"):
    """A depth tolerance as a float; ValueError unless it is a number >= 0 (+inf allowed)."""
    try:
        t = float(tol)
    except (ValueError, TypeError):
        t = math.nan
    if not t >= 0:
        raise ValueError("%s: %s must be a number >= 0, got %r" % (what, name, tol))
    return t


def _rig_inputs(what, depth, intrinsics, extrinsics, mask):
    """What every call that takes a rig's images checks first, nothing moved to the device -> (depth [B * V, H, W]: an image per
    row, body-major; intrinsics float64 [B * V, 4]; ext float32 [B, V, 12]; mask [B * V, H, W] or None)."""
    ext, batched = pack_extrinsics(extrinsics, what + ": extrinsics")
    B, V = ext.shape[:2]
    if V > ops.MAX_VIEWS:
        raise ValueError("%s: %d views, at most %d" % (what, V, ops.MAX_VIEWS))
    shape = tuple(getattr(depth, "shape", np.shape(depth)))
    if len(shape) != (4 if batched else 3) or shape[:-2] != ((B, V) if batched else (V,)):
        raise ValueError("%s: depth must be %s for extrinsics of %d bodies x %d views, got %s"
                         % (what, "[%d, %d, H, W]" % (B, V) if batched else "[%d, H, W]" % V, B, V, shape))
    k = _intrinsics_arg(what, intrinsics, ((4,), (V, 4), (B, V, 4)))
    flat = lambda a: None if a is None else a.reshape((B * V,) + tuple(a.shape[-2:]))      # noqa: E731 - [B * V, H, W]: an image per row
    if mask is not None and tuple(getattr(mask, "shape", np.shape(mask))) != shape:
        raise ValueError("%s: mask must have the depth's shape %s" % (what, shape))
    return (flat(depth if torch.is_tensor(depth) else np.asarray(depth)), np.broadcast_to(k, (B, V, 4)).reshape(B * V, 4), ext,
            flat(mask if mask is None or torch.is_tensor(mask) else np.asarray(mask)))


def _unproject_depth_views(depth, intrinsics, extrinsics, depth_scale=1.0, mask=None, z_range=None, max_step=None, drop_isolated=False, stride=1,
                           device=None, merge_tol=None, distortion=None):
    """`unproject_depth_views`, with the counts as the host read them and the extrinsics float32 [B, V, 12] as two more results -
    and, with a merge_tol, `seen` as a ninth.  Every ValueError is raised before the device is used."""
    what = "unproject_depth_views"
    if merge_tol is not None:
        merge_tol = _check_merge_tol(what, merge_tol)
    d, k, ext, m = _rig_inputs(what, depth, intrinsics, extrinsics, mask)
    rows = _depth_rows(what, d, k, ext, depth_scale, m, z_range, max_step, drop_isolated, stride, device, merge_tol, distortion)
    return rows[:7] + (ext,) + rows[7:]


def unproject_depth_views(depth, intrinsics, extrinsics, *, depth_scale=1.0, mask=None, z_range=None, max_step=None, drop_isolated=False, stride=1,
                          device=None, merge_tol=None, distortion=None):
    """The depth cameras of a rig -> ONE scan per body in the rig's frame (sh_depth_views_count, sh_depth_views_points;
    include/sh_kernels.h, "Depth views").  depth: [B, V, H, W], or [V, H, W] with extrinsics that have no batch axis (B = 1); fp32 or
    16-bit words as in `unproject_depth`, and depth_scale, mask (the depth's shape), z_range, max_step, drop_isolated and stride
    mean per image what they mean there.  intrinsics: (fx, fy, cx, cy) as [4], [V, 4] or [B, V, 4].  extrinsics: camera -> rig as
    [V, 3, 4] or [B, V, 3, 4] = (R | t), or 4 x 4 with the last row 0 0 0 1 (`pack_extrinsics`); rigid; an all-NaN matrix is an
    absent camera, which contributes nothing.  Every pixel's camera-frame point P and fp64 normal n are those of `unproject_depth`;
    the rows hold P' = R P + t (fp32, the header's order of operations) and n' = R n (fp64, rounded once), so a normal still faces
    its own camera.
    -> (points fp32 [B, M, 3], normals fp32 [B, M, 3], pixel int32 [B, M] = v * W + u within the row's view, view uint8 [B, M],
    counts int32 [B], view_first int32 [B, V + 1]: view v's rows are view_first[b, v]:view_first[b, v + 1]); M the largest count
    (at least 1); rows beyond a count are zeros, zeros, -1 and 255.  Rows are view-major, inside a view in tile / Z-order.  One
    host synchronisation.  Deterministic - the same bits for a body alone and inside any batch.  Not differentiable.  ValueError
    (before the device is used) for wrong shapes or dtypes, more than 32 views, fx / fy not finite and positive, stride < 1, a
    negative max_step, or extrinsics that are no rigid transforms.
    merge_tol: None - nothing more is launched -, or a depth tolerance >= 0 (ValueError when negative or NaN): the rows that a
    better-placed camera also measures within it are dropped (`views_overlap`, `merge_views`) and the six results are the merged
    ones.  That costs TWO host synchronisations instead of one: the kept counts are read as well.
    distortion: None, or the cameras' lenses as in `unproject_depth` - coefficients [k], [V, k] or [B, V, k], or a ready
    `CameraRays` of [V] or [B, V] cameras: the points come from the ray tables (sh_depth_views_rays_count / _points) and, with a
    merge_tol, the overlap pass projects through the lens model (sh_depth_views_rays_overlap).  A calibration that does not differ
    between the bodies is ONE table per camera, whatever B.  One resolution per rig."""
    points, normals, pixel, view, view_first, counts = _unproject_depth_views(depth, intrinsics, extrinsics, depth_scale, mask, z_range, max_step,
                                                                              drop_isolated, stride, device, merge_tol, distortion)[:6]
    return points, normals, pixel, view, counts, view_first


def _merge_rows(points, normals, pixel, view, counts, V, keep, seen):
    """A rig batch's planes under a keep plane (uint8 or bool [B, M]; the padding counts as dropped whatever it holds) -> (points,
    normals, pixel, view, view_first, counts, host_counts, seen or None), compacted (ops.scan_compact).  The kept counts are an
    integer sum in torch - exact - and reading them is the one synchronisation."""
    M = points.shape[1]
    live = torch.arange(M, device=points.device)[None, :] < counts[:, None]
    keep = ((keep != 0) & live).to(torch.uint8).contiguous()
    kept = keep.sum(1, dtype=torch.int32)
    host_counts = kept.cpu().numpy()                                                    # the one synchronisation
    most = int(host_counts.max()) if host_counts.size else 0
    p, n, pix, vw, sn, cnt, first = ops.scan_compact(points, normals, pixel, view, keep, counts, V, max(most, 1), most, seen)
    return p, n, pix, vw, first, cnt, host_counts, sn


def _rig_batch(what, scans):
    """ValueError unless `scans` is a rig batch made from depth images: `view`, `view_first`, `pixels`, normals and rig viewpoints."""
    if not (isinstance(scans, ScanBatch) and scans.view is not None and scans.view_first is not None and scans.pixels is not None
            and scans.normals is not None and scans.viewpoints is not None and scans.viewpoints.dim() == 3):
        raise ValueError("%s: scans must be a rig batch made from depth images (ScanBatch.from_depth(..., extrinsics=)); a cloud fused "
                         "elsewhere carries no images to compare" % what)
    return scans.view_first.shape[1] - 1


def views_overlap(scans, depth, intrinsics, extrinsics, *, tol, depth_scale=1.0, mask=None, z_range=None, distortion=None):
    """Which rows of a rig batch a better-placed camera also measures (sh_depth_views_overlap; include/sh_kernels.h, "Depth views:
    overlap").  scans: the rig batch `ScanBatch.from_depth(depth, intrinsics, device, extrinsics=extrinsics, ...)` made from THESE
    images - depth, intrinsics, extrinsics, depth_scale, mask and z_range as given there (max_step, drop_isolated and stride are
    not consulted).  Each row's point is projected into every other camera; that camera observes it when the nearest pixel is
    valid and its depth agrees with the point's within tol (projective association: no search).  Of the cameras that observe a
    row the one with the largest cos(theta) / d^2 under the row's own normal keeps it - depth noise grows with d^2 / cos(theta) -
    and on a tie the lower index.
    -> (keep bool [B, M]: False where another camera keeps the row, and in the padding; seen int32 [B, M] read as unsigned: bit c
    set where camera c observes the row, its own bit always).  One launch, nothing synchronised; fp32 throughout, deterministic.
    ValueError (before the device is used) for scans that are no rig batch or of another B or V, a tol that is negative or NaN,
    and what `unproject_depth_views` refuses in the images.
    distortion: None, or the lenses given to `from_depth` (`unproject_depth_views`): every point is projected through the lens
    model, and a point beyond a camera's fold-back limit is not observed by it (sh_depth_views_rays_overlap)."""
    what = "views_overlap"
    V = _rig_batch(what, scans)
    tol = _check_merge_tol(what, tol, "tol")
    d, k, ext, m = _rig_inputs(what, depth, intrinsics, extrinsics, mask)
    if ext.shape[:2] != (len(scans), V):
        raise ValueError("%s: the scans hold %d bodies x %d views, the extrinsics %d x %d" % ((what, len(scans), V) + ext.shape[:2]))
    d, k, m, near, far = _depth_inputs(what, d, k, m, z_range)
    rig = tuple(ext.shape[:2])
    cal = _calibration(what, distortion, k, rig[0], rig[1], d.shape[-2], d.shape[-1], scans.points.device)
    d, k, m = _depth_upload(d, k, m, scans.points.device)
    rays = {}
    if cal is not None:
        m = _ray_mask(cal, m, rig[0], rig[1], d.shape[-2], d.shape[-1])
        rays = dict(rays=cal[0]._planes(cal[1]))
    d = d.view(rig + tuple(d.shape[-2:]))
    seen, keep = ops.depth_views_overlap(d, k.view(rig + (4,)), torch.from_numpy(ext).to(d.device), scans.points, scans.normals, scans.view,
                                         scans.counts, tol, mask=None if m is None else m.view(d.shape), depth_scale=depth_scale, z_near=near,
                                         z_far=far, **rays)
    return keep.bool(), seen


def merge_views(scans, keep, seen=None):
    """A rig batch without the rows `keep` marks False (sh_scan_compact): a new rig ScanBatch with fresh points / normals / pixels /
    view / view_first / counts / host_counts - the kept rows in their old order, so still view-major and in tile order inside a
    view -, `viewpoints` carried over, perm None, and `seen` (int32 [B, M], `views_overlap`'s) compacted with them as
    `ScanBatch.seen` when given.  keep: bool or integer [B, M], a tensor or a host array; what it holds in the padding is not
    read.  One host synchronisation, to read the kept counts (`keep.sum(1)`, exact).  chamfer, align, fit_scan and register_scan
    read the result like any rig batch.  ValueError for scans that are no rig batch made from depth images, or a keep / seen of
    another shape."""
    what = "merge_views"
    V = _rig_batch(what, scans)
    shape = tuple(scans.points.shape[:2])
    planes = []
    for name, t in (("keep", keep), ("seen", seen)):
        if t is not None:
            t = t.detach() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
            if tuple(t.shape) != shape or t.is_floating_point() or t.is_complex():
                raise ValueError("%s: %s must be a bool or integer array of the scans' shape %s, got %s %s" % (what, name, shape, t.dtype, tuple(t.shape)))
        planes.append(t)
    keep, seen = planes
    dev = scans.points.device
    if seen is not None:
        seen = seen.to(dev)
        seen = (seen if seen.dtype in ops._SEEN else seen.to(torch.int32)).contiguous()
    p, n, pix, vw, first, cnt, host_counts, sn = _merge_rows(scans.points.contiguous(), scans.normals.contiguous(), scans.pixels.contiguous(),
                                                            scans.view.contiguous(), scans.counts, V, keep.to(dev), seen)
    return ScanBatch._from_parts(p, cnt, host_counts, None, n, viewpoints=scans.viewpoints, pixels=pix, view=vw, view_first=first, seen=sn)


class DepthField:
    """What B depth images say about where the body is NOT, resident on the device (sh_depth_field; include/sh_kernels.h, "Depth
    field"): `cls` uint8 [B, H, W] - 2 SURFACE (a valid pixel in the sense of `unproject_depth`), 0 EMPTY (a reading that is not
    the surface, at or beyond the near end of z_range: the sensor saw through here), 1 UNKNOWN (no reading, or something nearer
    than z_range) -, `z` fp32 [B, H, W] the surface depth (0 elsewhere), `nearest` int32 [B, H, W] the nearest pixel that is not
    EMPTY as v * W + u (exact, ties to the smallest index, -1 when the image has none), `intrinsics` fp32 [B, 4] and `shape` =
    (H, W).  `free_space` reads it; made once per image batch by `from_depth`.
    A RIG field (`from_depth(..., extrinsics=)`) holds the V cameras of every body: the planes are [B, V, H, W], `intrinsics`
    [B, V, 4], `extrinsics` fp32 [B, V, 12] on the device (camera -> rig, `pack_extrinsics`' layout; a NaN row: an absent camera)
    and `views` = V; `len` is still B and `shape` (H, W).  Without extrinsics both members are None.
    `rays`: None, or the cameras' lenses as a `CameraRays` (`from_depth(..., distortion=)`): `free_space` then projects through the
    lens model and takes the silhouette rays from the tables."""

    def __init__(self, cls, z, nearest, intrinsics, extrinsics=None, rays=None, rays_lead=None):
        self.cls, self.z, self.nearest, self.intrinsics, self.extrinsics = cls, z, nearest, intrinsics, extrinsics
        self.rays, self._rays_lead = rays, rays_lead
        self.views = None if extrinsics is None else int(extrinsics.shape[1])
        self.shape = tuple(cls.shape[-2:])

    @classmethod
    def from_depth(cls, depth, intrinsics, device=None, *, extrinsics=None, depth_scale=1.0, mask=None, z_range=None, distortion=None):
        """depth, intrinsics, depth_scale, mask, z_range and device as in `unproject_depth`, with its checks and ValueErrors (raised
        before the device is used).  Two launches, no host synchronisation.  Deterministic - the same bits for an image alone and
        inside any batch.  RuntimeError for an image side above 16384.
        extrinsics: None, or a rig's camera -> rig transforms [V, 3, 4] / [B, V, 3, 4] with depth [V, H, W] / [B, V, H, W] and
        intrinsics [4], [V, 4] or [B, V, 4] as in `unproject_depth_views` (its checks and ValueErrors): a rig field, made by the
        same two launches over the B * V images.
        distortion: None, or the lenses as in `unproject_depth` / `unproject_depth_views` (their checks and ValueErrors).  The
        field's planes live in pixel space and are made by the same two launches; the table is kept as `rays`, and a pixel
        without a ray is classified as a masked one is."""
        what = "DepthField.from_depth"
        ext = None
        if extrinsics is not None:
            depth, intrinsics, ext, mask = _rig_inputs(what, depth, intrinsics, extrinsics, mask)
        d, k, m, near, far = _depth_inputs(what, depth, intrinsics, mask, z_range)
        B, V = (d.shape[0], 0) if ext is None else tuple(ext.shape[:2])
        cal = _calibration(what, distortion, k, B, V, d.shape[-2], d.shape[-1], device if device is not None or not d.is_cuda else d.device)
        d, k, m = _depth_upload(d, k, m, device)
        if cal is not None:
            m = _ray_mask(cal, m, B, V, d.shape[-2], d.shape[-1])
        lens = {} if cal is None else dict(rays=cal[0], rays_lead=cal[1])
        planes = ops.depth_field(d, k, mask=m, depth_scale=depth_scale, z_near=near, z_far=far)
        if ext is None:
            return cls(*planes, k, **lens)
        rig = tuple(ext.shape[:2])                                          # the same call over the B * V images, reshaped
        return cls(*(p.view(rig + tuple(p.shape[-2:])) for p in planes), k.view(rig + (4,)), torch.from_numpy(ext).to(d.device), **lens)

    def __len__(self):
        return self.cls.shape[0]

    def select(self, sl):
        """The images `sl` (a slice; of a rig field: the bodies) as a DepthField sharing this one's memory."""
        out = DepthField(self.cls[sl], self.z[sl], self.nearest[sl], self.intrinsics[sl], None if self.extrinsics is None else self.extrinsics[sl])
        if self.rays is not None:                                           # tables per body are cut with them; one table per camera is shared
            per_body = self._rays_lead == ((len(self), self.views) if self.views else (len(self),)) and self.rays.lead == self._rays_lead
            out.rays = self.rays.select(sl) if per_body else self.rays
            out._rays_lead = (len(out),) + self._rays_lead[1:] if per_body else self._rays_lead
        return out

    def _lens(self):
        """What ops takes as rays=: None, or (table, coefficients, limit)."""
        return None if self.rays is None else self.rays._planes(self._rays_lead)


def nearest(q, t, q_count=None, t_count=None, t_mask=None, chunks=0):
    """For every query q[b, j] its nearest target in t[b]: (idx int32 [B, nq], d2 fp32 [B, nq]), d2 the squared distance in the
    difference form of sh_kernels.h, idx the lowest index on an exact tie.  q_count / t_count [B]: live rows per body (None =
    all); t_mask [nt] or [B, nt]: False = target not allowed.  No allowed target: idx -1, d2 +inf; queries beyond q_count:
    idx -1, d2 0.  chunks: how many ranges the targets are split into (0 = chosen by the library; every split gives the same
    bits).  Not differentiable."""
    return ops.nearest_points(q.detach(), t.detach(), q_count, t_count, t_mask, chunks=chunks)


class FaceTable:
    """The model's triangles for the surface search: `faces` int32 [nF, 3] on the device, one table for every body of a batch;
    `n` is the number of model vertices the indices may address (the decoder's dummy row, row n, is not among them).
    `vf_ptr` int32 [n + 1] / `vf_idx` int32 [3 nF] are the vertex-to-face incidence (CSR, built once here on the host): the faces
    that name vertex v are vf_idx[vf_ptr[v]:vf_ptr[v + 1]], in ascending face order - what `vertex_normals` walks.
    ValueError unless the table is an integer array [nF, 3] with 0 <= index < n and no face that names a vertex twice."""

    def __init__(self, faces, n, device):
        f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
        if f.dtype.kind not in "iu":
            raise ValueError("FaceTable: faces must be integers, got %s" % f.dtype)
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("FaceTable: faces must be [nF, 3], got %s" % (f.shape,))
        n = int(n)
        f = f.astype(np.int64)
        if f.size and (f.min() < 0 or f.max() >= n):
            raise ValueError("FaceTable: face indices must lie in [0, %d) (the dummy row is not a vertex); got [%d, %d]"
                             % (n, f.min(), f.max()))
        if ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any():
            raise ValueError("FaceTable: a face names the same vertex twice")
        self.n = n
        self.faces = torch.from_numpy(np.ascontiguousarray(f.astype(np.int32))).to(torch.device(device))
        flat = f.reshape(-1)
        order = np.argsort(flat, kind="stable")                            # stable: a vertex's faces stay in ascending face order
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(flat, minlength=n), out=ptr[1:])
        self.vf_ptr = torch.from_numpy(ptr.astype(np.int32)).to(self.faces.device)
        self.vf_idx = torch.from_numpy((order // 3).astype(np.int32)).to(self.faces.device)

    def __len__(self):
        return self.faces.shape[0]


def _face_table(faces, n, device):
    if isinstance(faces, FaceTable):
        if faces.n > n:
            raise ValueError("face table made for %d vertices, the model has %d" % (faces.n, n))
        return faces
    return FaceTable(faces, n, device)


def vertex_normals(x, faces, n=None):
    """Area-weighted unit vertex normals of every body, fp32 [B, n, 3] (sh_vertex_normals: the fp32 expression of sh_kernels.h,
    one thread per vertex over its incident faces in ascending face order; deterministic).  x [B, rows, 3]; faces: a FaceTable or
    an integer array [nF, 3], oriented counter-clockwise seen from outside for outward normals; n as in `chamfer` (None = rows -
    1).  A vertex in no face, or whose faces' cross products cancel, gets the zero vector.  The vertex mask plays no part.  Not
    differentiable."""
    x = x.detach()
    rows = ops._points(x, "scan.vertex_normals")[1]
    ft = _face_table(faces, rows if isinstance(faces, FaceTable) else (rows - 1 if n is None else int(n)), x.device)
    return ops.vertex_normals(x, ft.faces, ft.vf_ptr, ft.vf_idx, ft.n)


def face_normals(x, faces, n=None):
    """Unit face normals of every body, fp32 [B, nF, 3] (sh_face_normals: the fp32 expression of sh_kernels.h, one thread per
    face; deterministic).  x, faces and n as in `vertex_normals`; faces oriented counter-clockwise seen from outside give outward
    normals.  A face without area gets the zero vector.  The vertex mask plays no part.  Not differentiable."""
    x = x.detach()
    rows = ops._points(x, "scan.face_normals")[1]
    ft = _face_table(faces, rows if isinstance(faces, FaceTable) else (rows - 1 if n is None else int(n)), x.device)
    return ops.face_normals(x, ft.faces, ft.n)


def _cos_grazing(what, grazing_angle):
    """A grazing angle in degrees, checked -> the bound sh_vertex_visibility holds the normal's component along the line of sight
    against; 90 is an exact 0 (a zero normal passes there, and only there)."""
    a = float(grazing_angle)
    if not 0.0 < a <= 90.0:
        raise ValueError("%s: grazing_angle must lie in (0, 90] degrees, got %r" % (what, grazing_angle))
    return 0.0 if a == 90.0 else math.cos(math.radians(a))


def _view_arg(what, viewpoints, B, device, rig=False):
    """Per-body viewpoints as the kernels take them: host [3] / [B, 3] (a NaN row = no viewpoint) or an fp32 device tensor [B, 3]
    or [B, V, 3] (a rig of 1 <= V <= 32 sensors; a NaN row = an absent one) -> contiguous fp32 [B, 3] or [B, V, 3] on `device`
    (None: where it is).  A HOST array of rank 3 is refused here, as it always was: a rig's viewpoints reach the kernels as a
    device tensor - what a rig batch carries.  rig=True (ScanBatch's rig_viewpoints=): a rig is meant, host [V, 3] (one rig for
    every body) or [B, V, 3] is taken, inf is refused.  ValueError on any other shape."""
    v = viewpoints
    rig_ok = lambda shape: len(shape) == 3 and shape[0] == B and 1 <= shape[1] <= ops.MAX_VIEWS and shape[2] == 3      # noqa: E731
    if torch.is_tensor(v) and v.is_cuda:
        if v.dtype != torch.float32 or not (tuple(v.shape) == (B, 3) and not rig or rig_ok(tuple(v.shape))):
            raise ValueError("%s: device viewpoints must be fp32 [%d, 3] or [%d, V <= %d, 3], got %s %s"
                             % (what, B, B, ops.MAX_VIEWS, v.dtype, tuple(v.shape)))
        return v.detach().contiguous()
    if torch.is_tensor(v):
        v = v.detach().numpy()
    try:
        a = np.asarray(v, dtype=np.float32)
    except (ValueError, TypeError):
        a = None
    if rig and a is not None and a.ndim == 2:
        a = np.broadcast_to(a, (B,) + a.shape)
    if a is None or not (rig_ok(a.shape) and not np.isinf(a).any() if rig else a.shape in ((3,), (B, 3))):
        raise ValueError("%s: viewpoints must be %s, got %s"
                         % (what, "[V, 3] or [%d, V <= %d, 3] without inf" % (B, ops.MAX_VIEWS) if rig else
                            "[3] or [%d, 3] (a rig's [%d, V <= %d, 3]: an fp32 device tensor)" % (B, B, ops.MAX_VIEWS),
                            "shape %s" % (a.shape,) if a is not None else type(v).__name__))
    out = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (B, 3)) if a.ndim < 3 else a))
    return out if device is None else out.to(device)


def _visibility(x, ft, view, v_mask, tn, cos_g, chunks=0, out=None, seen=False):
    """The one place that picks the visibility kernel by the viewpoints' rank: [B, 3] -> sh_vertex_visibility (launches and bits as
    ever), [B, V, 3] -> sh_vertex_visibility_views.  seen=True (a rig only): (vis, the per-view bits)."""
    if seen and view.dim() != 3:
        raise ValueError("visible_vertices: return_seen needs rig viewpoints [B, V, 3], got [B, 3]")
    rig = view.dim() == 3
    return ops._visibility("vertex_visibility_views" if rig else "vertex_visibility", rig, x, ft.faces, ft.n, view, v_mask, tn, cos_g, chunks,
                           out, seen)


def _move_viewpoints(view, packed, out=None):
    """Viewpoints [B, 3] or [B, V, 3] under the poses `packed` [B, 12] (sh_transform_points, one row per sensor; a NaN row stays
    NaN) -> the same shape; out: a tensor of that shape to write into."""
    rows = view[:, None, :] if view.dim() == 2 else view
    moved = ops.transform_points(rows, None, packed, out=None if out is None else (out[:, None, :] if out.dim() == 2 else out))
    return moved[:, 0] if view.dim() == 2 else moved


def visible_vertices(x, faces, viewpoints, n=None, vertex_mask=None, grazing_angle=None, chunks=0, return_seen=False):
    """The model vertices a sensor sees: bool [B, n] on the device (sh_vertex_visibility; include/sh_kernels.h, "Vertex
    visibility").  Vertex i of body b is visible when it is active (vertex_mask [n] or [B, n], False = not visible), the open
    segment from it to the body's viewpoint meets no triangle of `faces` other than those that name i - every triangle occludes,
    masked or not - and, with grazing_angle (degrees in (0, 90]), its normal (`vertex_normals(x, faces)`) lies within that angle
    of the line of sight; a zero normal passes only at 90.  Without grazing_angle no normals are computed.  x [B, rows, 3]; faces:
    a FaceTable or an integer array [nF, 3]; n as in `chamfer` (None = rows - 1).  viewpoints: host [3] / [B, 3] or an fp32 device
    tensor [B, 3], in the frame of x; a body whose row holds a NaN has no viewpoint and all its active vertices are visible.
    chunks: the split of the face range (0 = chosen by the library; every split gives the same bits).  Brute force, O(n nF) per
    body with early exits.  Deterministic, not differentiable.  ValueError for a wrong viewpoint shape or a grazing_angle outside
    (0, 90].
    A rig: viewpoints an fp32 device tensor [B, V, 3], 1 <= V <= 32 - a rig batch's `viewpoints`; a host array of rank 3 stays
    refused, as before rigs existed - -> visible from AT LEAST ONE of the V sensors
    (sh_vertex_visibility_views: one sweep over the faces, not V).  A NaN row is an absent sensor; a body whose rows are all NaN
    has no viewpoint.  return_seen=True (a rig only) -> (visible, seen): seen [B, n] holds the 32-bit word whose bit v says that
    sensor v alone sees the vertex - exactly what the call with viewpoints[:, v] returns - as torch.uint32 where torch has it,
    else the same bits as int32."""
    cos_g = None if grazing_angle is None else _cos_grazing("visible_vertices", grazing_angle)
    if torch.is_tensor(x) and x.dim() == 3:
        viewpoints = _view_arg("visible_vertices", viewpoints, x.shape[0], None)    # the shape check needs no device
        x = x.detach()
    B, rows, _ = ops._points(x, "scan.visible_vertices")
    view = viewpoints.to(x.device)
    ft = _face_table(faces, rows if isinstance(faces, FaceTable) else (rows - 1 if n is None else int(n)), x.device)
    tn = None if cos_g is None else ops.vertex_normals(x, ft.faces, ft.vf_ptr, ft.vf_idx, ft.n)
    got = _visibility(x, ft, view, vertex_mask, tn, 0.0 if cos_g is None else cos_g, chunks=chunks, seen=return_seen)
    if not return_seen:
        return got.bool()
    return got[0].bool(), got[1].view(torch.uint32) if hasattr(torch, "uint32") else got[1]


def _cos_min(what, normal_angle):
    """A gate's angle in degrees, checked -> the bound the kernels hold the fp32 dot product of two normals against; 180 opens the
    gate (-inf)."""
    a = float(normal_angle)
    if not 0.0 < a <= 180.0:
        raise ValueError("%s: normal_angle must lie in (0, 180] degrees, got %r" % (what, normal_angle))
    return -math.inf if a == 180.0 else math.cos(math.radians(a))


def _query_normals(tn, rows):
    """Vertex normals [B, n, 3] as the model -> scan search takes them, [B, rows, 3]: every row of the model is a query there, and
    the rows behind the vertices (the decoder's dummy row) carry the zero normal."""
    return tn if rows == tn.shape[1] else torch.nn.functional.pad(tn, (0, 0, 0, rows - tn.shape[1]))


def nearest_surface(q, x, faces, q_count=None, vertex_mask=None, chunks=0, cull=True, n=None, q_normals=None, normal_angle=None):
    """For every scan point q[b, j] the closest point of body b's triangles: (face int32 [B, nq], d2 fp32 [B, nq], uv fp32
    [B, nq, 2]), exact in the fp32 expression of sh_kernels.h - the lexicographic minimum of (d2, face) over all target
    triangles, uv the barycentric weights (l1, l2) of the foot point on that face (l0 = 1 - l1 - l2).  x [B, rows, 3]; faces: a
    FaceTable (its n says how many leading rows of x are vertices) or an integer array [nF, 3], validated against n - as in
    `chamfer`, n=None means rows - 1 (the decoder's dummy row is no vertex); pass n=rows for a bare vertex tensor.  vertex_mask [n]
    or [B, n]: a triangle with a masked corner is no target.  No target: face -1, d2 +inf; points beyond q_count: face -1, d2 0.
    cull=True starts from the nearest vertex (one sh_nearest_points search) and tests only the triangles whose bounding sphere
    reaches inside the best distance so far; cull=False tests every pair - same bits, many times the work.  chunks: the split of
    the triangle range (0 = chosen by the library; every split gives the same bits).  Not differentiable.

    q_normals [B, >= nq, 3] with normal_angle (degrees in (0, 180]; both or neither): the bare gated search
    (sh_nearest_surface_gated) - only the triangles whose face normal (`face_normals(x, faces)`) lies within that angle of the
    point's normal are candidates; a point with none gets face -1, d2 +inf, uv 0.  cull=True is then bounded by the gated search
    over the face centres instead of the nearest vertex.  180 opens the gate: the ungated bits."""
    q, x = q.detach(), x.detach()
    rows = ops._points(x, "scan.nearest_surface")[1]
    ft = _face_table(faces, rows if isinstance(faces, FaceTable) else (rows - 1 if n is None else int(n)), x.device)
    if (q_normals is None) != (normal_angle is None):
        raise ValueError("nearest_surface: q_normals and normal_angle come together")
    if normal_angle is not None:
        cos_min = _cos_min("nearest_surface", normal_angle)
        fn = ops.face_normals(x, ft.faces, ft.n)
        return ops.nearest_surface(q, x, ft.faces, ft.n, q_count, vertex_mask, None, chunks=chunks, cull=cull, gate=(q_normals.detach(), fn, cos_min))
    bound = None
    if cull:
        bound = ops.nearest_points(q, x, q_count=q_count, t_mask=vertex_mask, nt=ft.n)[1]
    return ops.nearest_surface(q, x, ft.faces, ft.n, q_count, vertex_mask, bound, chunks=chunks, cull=cull)


def closest_points(x, faces, face, uv):
    """The foot points [B, M, 3] that `nearest_surface` found, rebuilt from (face, uv) in plain torch: a + l1 (b - a) + l2 (c - a)
    on the face's corners; rows with face -1 give zeros.  Differentiable w.r.t. x (the weights are constants)."""
    f = faces.faces if isinstance(faces, FaceTable) else torch.as_tensor(faces, device=x.device)
    B = x.shape[0]
    corners = f.long()[face.clamp_min(0).long()]                            # [B, M, 3]
    ar = torch.arange(B, device=x.device)[:, None]
    a, b, c = (x[ar, corners[:, :, k]] for k in range(3))
    p = a + uv[:, :, 0:1] * (b - a) + uv[:, :, 1:2] * (c - a)
    return torch.where((face >= 0)[:, :, None], p, torch.zeros_like(p))


VERTEX, VERTEX_GATED, SURFACE, SURFACE_GATED = "vertex", "vertex, gated", "surface", "surface, gated"


def _robust_arg(what, robust, robust_scale):
    """`robust` / `robust_scale` checked -> None (no robust term: the plain kernels) or (form id, scale2 = sigma^2) as the `_robust`
    entry points take them.  ValueError on an unknown name, a scale without a name, a name without a scale, or a scale that is
    not a positive finite number."""
    if robust is None:
        if robust_scale is not None:
            raise ValueError("%s: robust_scale given without robust (one of %s)" % (what, sorted(ops.ROBUST_FORMS)))
        return None
    if not isinstance(robust, str) or robust not in ops.ROBUST_FORMS:
        raise ValueError("%s: robust must be None or one of %s, got %r" % (what, sorted(ops.ROBUST_FORMS), robust))
    if robust_scale is None:
        raise ValueError("%s: robust=%r needs robust_scale (sigma, in the model's normalised units)" % (what, robust))
    try:
        sigma = float(robust_scale)
    except (TypeError, ValueError):
        sigma = math.nan
    scale2 = sigma * sigma
    if not (sigma > 0.0 and math.isfinite(scale2) and float(np.float32(scale2)) > 0.0 and math.isfinite(float(np.float32(scale2)))):
        raise ValueError("%s: robust_scale must be a positive finite number, got %r" % (what, robust_scale))
    return ops.ROBUST_FORMS[robust], scale2


def robust_weights(d2, robust, robust_scale, trunc=None):
    """The per-pair weights of recorded squared distances d2 under a robust term, for inspection: w = d rho / d u at u = d2 in the
    fp32 expressions of include/sh_kernels.h ("Robust terms") for the kept pairs (d2 < trunc^2, all finite ones without trunc),
    0 for the truncated ones.  Plain torch in fp32 on whatever device d2 lives on; the kernels compute the same expressions
    themselves and never call this.  robust=None gives 1 for every kept pair.  Errors as in `chamfer`."""
    rb = _robust_arg("robust_weights", robust, robust_scale)
    if trunc is not None and not float(trunc) > 0.0:
        raise ValueError("robust_weights: trunc must be > 0")
    u = torch.as_tensor(d2, dtype=torch.float32)
    tau2 = torch.tensor(math.inf if trunc is None else float(trunc) ** 2, dtype=torch.float32, device=u.device)
    one = torch.ones_like(u)
    if rb is None:
        w = one
    else:
        s2 = torch.tensor(rb[1], dtype=torch.float32, device=u.device)
        if rb[0] == ops.ROBUST_FORMS["geman-mcclure"]:
            t = s2 / (s2 + u)
            w = t * t
        else:
            inside = u <= s2
            w = torch.where(inside, one, torch.sqrt(s2 / torch.where(inside, one, u)))
    return torch.where(u < tau2, w, torch.zeros_like(u))


class _MatchPlan:
    """What one call of `chamfer` or `align` matches, resolved once from its arguments - every check of them included, in the order
    the docstrings promise - and the one routine, `search`, that runs the searches of a forward pass or an ICP iteration.

    n, rows, v_mask, mask_sb, tau2, w: the arguments as the kernels take them; `scans` the ScanBatch.  cos_min: the gate's bound, or
    None without a gate.  surface: the FaceTable of the surface distance, or None.  normals: the FaceTable the vertex normals come
    from (a gate's, or with step="plane" the table the step's normals need), or None.  recorded: the table `matches` receives as
    `normal_faces` - `normals`, else `surface`, else with record=True a given normal_faces - or None.  kind: the scan -> model
    partner, one of VERTEX, VERTEX_GATED, SURFACE (bounded by the vertex search), SURFACE_GATED (the face-normal gate).  An
    array becomes a FaceTable here, once; a FaceTable is used as it is.  pair: what `_check_pair` returned; `chamfer`
    takes no pose step and leaves `step` alone.

    visibility: None, or "viewpoint" - then `see(x, view)` replaces v_mask by the given mask AND the vertices the sensor at `view`
    sees (sh_vertex_visibility on `vis_table`: visibility_faces, else faces, else normal_faces), with mask_sb = n; searches, loss,
    gradient, moments and `pose_update` read it as they read a given mask.  cos_g: the grazing bound, or None.

    robust: None, or (form id, scale2) of the robust term (`_robust_arg`) - what `loss`, the backward pass and `align`'s pose steps
    hand to the wrappers of ops; None takes the plain entry points."""

    def __init__(self, what, x, pair, vertex_mask, trunc, w_model_to_scan, faces, normal_angle, normal_faces, gate_on, step="point", record=False,
                 visibility=None, visibility_faces=None, grazing_angle=None, robust=None, robust_scale=None):
        self.scans, B, self.rows, self.n = pair
        self.check_visibility(what, visibility, visibility_faces, faces, normal_faces, grazing_angle, self.scans)
        self.w = float(w_model_to_scan)
        if not self.w >= 0.0:
            raise ValueError("%s: w_model_to_scan must be >= 0" % what)
        if trunc is not None and not float(trunc) > 0.0:
            raise ValueError("%s: trunc must be > 0" % what)
        self.tau2 = math.inf if trunc is None else float(trunc) ** 2
        self.robust = _robust_arg(what, robust, robust_scale)
        self.v_mask, self.mask_sb = ops._mask_arg(vertex_mask, B, self.n, x.device)

        def table(f):
            return _face_table(f, self.n, x.device)

        def same_n(ft, name="the face table"):
            if ft.n != self.n:
                raise ValueError("%s: %s was made for %d vertices, the model has %d" % (what, name, ft.n, self.n))

        self.surface = table(faces) if gate_on == "surface" and faces is not None else None
        self.cos_min = self.check_gate(what, gate_on, normal_angle, faces, self.scans, trunc)
        self.normals = None
        if self.cos_min is not None:                                                # the face-normal gate of the surface search
            self.normals = self.surface if normal_faces is None else table(normal_faces)
            same_n(self.normals)
            same_n(self.surface)
        elif normal_angle is not None:                                              # the gate on vertex normals
            self.cos_min = _cos_min(what, normal_angle)
            if faces is not None:
                raise ValueError("%s: normal_angle together with faces= (the surface distance) is not built for the gate on vertex normals; "
                                 "gate_on='surface' gates the surface search by the face's normal" % what)
            if self.scans.normals is None:
                raise ValueError("%s: normal_angle needs scan normals (ScanBatch(..., normals=))" % what)
            if normal_faces is None:
                raise ValueError("%s: normal_angle needs the model's triangles (normal_faces=, a FaceTable or an integer array)" % what)
            if trunc is None:
                raise ValueError("%s: normal_angle needs trunc (a point with no compatible partner counts as truncated; without trunc "
                                 "the loss would be infinite)" % what)
            self.normals = table(normal_faces)
            same_n(self.normals, "normal_faces")
        elif faces is not None:
            self.surface = table(faces)
        if step not in ("point", "plane"):
            raise ValueError("%s: step must be 'point' or 'plane'" % what)
        if step == "plane" and self.normals is None and (self.surface is None or self.w > 0.0):   # vertex normals are read, no gate brought a table
            if self.surface is None and normal_faces is None:
                raise ValueError("%s: step='plane' on vertex pairs needs the model's triangles (normal_faces=, a FaceTable or an integer array)" % what)
            self.normals = self.surface if self.surface is not None else table(normal_faces)
            same_n(self.normals)
        self.recorded = self.normals if self.normals is not None else self.surface
        if self.recorded is None and record and normal_faces is not None:
            self.recorded = table(normal_faces)
        self.kind = ((VERTEX, VERTEX_GATED), (SURFACE, SURFACE_GATED))[self.surface is not None][self.cos_min is not None]
        self.visibility, self.vis_table, self.cos_g, self.vis_tn = visibility, None, None, None
        if visibility is not None:
            self.given_mask = self.v_mask
            self.cos_g = None if grazing_angle is None else _cos_grazing(what, grazing_angle)
            vf = visibility_faces if visibility_faces is not None else (faces if faces is not None else normal_faces)
            if vf is faces and self.surface is not None:                            # a table already made from the same argument serves
                self.vis_table = self.surface
            elif vf is normal_faces and self.normals is not None and self.normals is not self.surface:
                self.vis_table = self.normals
            else:
                self.vis_table = table(vf)
            same_n(self.vis_table, "visibility_faces")

    @staticmethod
    def check_visibility(what, visibility, visibility_faces, faces, normal_faces, grazing_angle, scans):
        """The checks of `visibility` that need no device: ValueError on an unknown value, and for "viewpoint" on what it needs and
        lacks (per-body viewpoints on the scans, a face table), or on a grazing_angle outside (0, 90]."""
        if visibility not in (None, "viewpoint"):
            raise ValueError("%s: visibility must be None or 'viewpoint', got %r" % (what, visibility))
        if visibility is None:
            return
        if grazing_angle is not None:
            _cos_grazing(what, grazing_angle)
        if isinstance(scans, ScanBatch) and scans.viewpoints is None or not isinstance(scans, ScanBatch):
            why = getattr(scans, "viewpoints_error", None)
            raise ValueError("%s: visibility='viewpoint' needs the sensor's position per body (ScanBatch(..., viewpoints=[3] or [B, 3]), or a rig's: rig_viewpoints= / from_depth(extrinsics=))%s"
                             % (what, "; the viewpoints given were not kept: %s" % why if why else ""))
        if visibility_faces is None and faces is None and normal_faces is None:
            raise ValueError("%s: visibility='viewpoint' needs the model's triangles (visibility_faces=, faces= or normal_faces=)" % what)

    def see(self, x, view, out=None, static_x=False):
        """Recompute the mask for the model points x seen from `view` fp32 [B, 3] (or a rig's [B, V, 3]): v_mask = given mask AND visible, uint8 [B, n].
        static_x: x does not change between calls of this plan, so the facing test's normals are computed once."""
        ft, tn = self.vis_table, None
        if self.cos_g is not None:
            tn = self.vis_tn
            if tn is None:
                tn = ops.vertex_normals(x, ft.faces, ft.vf_ptr, ft.vf_idx, ft.n)
                self.vis_tn = tn if static_x else None
        self.v_mask = _visibility(x, ft, view, self.given_mask, tn, 0.0 if self.cos_g is None else self.cos_g, out=out)
        self.mask_sb = self.n
        return self.v_mask

    @staticmethod
    def check_gate(what, gate_on, normal_angle, faces, scans, trunc):
        """The checks of `gate_on` that need no device: ValueError on an unknown value, and for "surface" on whatever it needs and
        lacks (normal_angle, faces=, scan normals, trunc - each named).  -> the face-normal gate's cos_min, None for "vertices"."""
        if gate_on not in ("vertices", "surface"):
            raise ValueError("%s: gate_on must be 'vertices' or 'surface', got %r" % (what, gate_on))
        if gate_on != "surface":
            return None
        if normal_angle is None:
            raise ValueError("%s: gate_on='surface' needs normal_angle (degrees)" % what)
        cos_min = _cos_min(what, normal_angle)
        if faces is None:
            raise ValueError("%s: gate_on='surface' needs faces= (the model's triangles: the gate is on the face's normal)" % what)
        if isinstance(scans, ScanBatch) and scans.normals is None:
            raise ValueError("%s: gate_on='surface' needs scan normals (ScanBatch(..., normals=))" % what)
        if trunc is None:
            raise ValueError("%s: gate_on='surface' needs trunc (a point with no compatible face counts as truncated; without trunc "
                             "the loss would be infinite)" % what)
        return cos_min

    def search(self, x, scans, normals=(None, None, None), out=(None, None, None), chunks=0, cull=True, vertex_matches=True):
        """The searches of one forward pass or ICP iteration between the model points x and `scans` (the plan's, or those under a
        pose) -> the `matches` dict.  By kind, in launch order:

            VERTEX          nearest_points(s, x)                                                  |  w > 0: nearest_points(x, s)
            VERTEX_GATED    vertex_normals, the same under the gate (scan normals, tn, cos_min)    |  under (tn padded to rows, scan normals, cos_min)
            SURFACE         the vertex search, nearest_surface(bound = its d2; None with cull=False) |  ungated
            SURFACE_GATED   face_normals, nearest_surface(gate=, bound=None), vertex_normals if     |  gated as above; then, with vertex_matches,
                            w > 0 or vertex_matches                                                |  the gated vertex search, last

        normals: (tn, qn, fn) - vertex normals, their padded form and face normals - where the caller has them already (x fixed);
        what is None is computed here when it is read.  out: ((idx, d2) scan -> model, (face, d2, uv), (idx, d2) model -> scan)
        buffers to fill; None allocates.  vertex_matches: whether a SURFACE_GATED pass records vertex matches at all."""
        s, cnt, n, w, v_mask, cos_min, surf = scans.points, scans.counts, self.n, self.w, self.v_mask, self.cos_min, self.surface
        tn, qn, fn = normals
        sm, sf, ms = out
        idx_sm = d2_sm = idx_ms = d2_ms = None

        def model_normals():
            nonlocal tn, qn
            if tn is None:
                tn = ops.vertex_normals(x.detach(), self.normals.faces, self.normals.vf_ptr, self.normals.vf_idx, n)
            if qn is None and w > 0.0:
                qn = _query_normals(tn, self.rows)

        if self.kind == SURFACE_GATED:
            if fn is None:
                fn = ops.face_normals(x.detach(), surf.faces, n)
            found = ops.nearest_surface(s, x, surf.faces, n, cnt, v_mask, None, chunks=chunks, cull=cull, out=sf, gate=(scans.normals, fn, cos_min))
            if w > 0.0 or vertex_matches:
                model_normals()
        else:
            if self.kind == VERTEX_GATED:
                model_normals()
            idx_sm, d2_sm = ops.nearest_points(s, x, q_count=cnt, t_mask=v_mask, nt=n, chunks=chunks, out=sm,
                                               gate=None if cos_min is None else (scans.normals, tn, cos_min))
            if surf is not None:                                                    # the vertex distance bounds the surface search
                found = ops.nearest_surface(s, x, surf.faces, n, cnt, v_mask, d2_sm if cull else None, chunks=chunks, cull=cull, out=sf)
        if w > 0.0:                                                                 # all rows are queries: [B, rows] as the kernels index it
            idx_ms, d2_ms = ops.nearest_points(x, s, t_count=cnt, chunks=chunks, out=ms, gate=None if cos_min is None else (qn, scans.normals, cos_min))
        if self.kind == SURFACE_GATED and vertex_matches:                           # the gated VERTEX matches, for `pose_update`
            idx_sm, d2_sm = ops.nearest_points(s, x, q_count=cnt, t_mask=v_mask, nt=n, chunks=chunks, out=sm, gate=(scans.normals, tn, cos_min))
        m = dict(x=x.detach(), n=n, v_mask=v_mask, mask_sb=self.mask_sb, tau2=self.tau2, w_ms=w, idx_sm=idx_sm, d2_sm=d2_sm, idx_ms=idx_ms,
                 d2_ms=d2_ms, tn=tn, normal_faces=self.recorded)
        if surf is not None:
            m.update(face=found[0], d2_surface=found[1], uv=found[2], faces=surf.faces)
        return m

    def loss(self, m, scans, out=None):
        """sh_chamfer_fwd on what `search` found -> (loss [B], counts)."""
        return ops.chamfer_fwd(m["d2_sm"] if self.surface is None else m["d2_surface"], scans.counts, m["d2_ms"], self.rows, self.n, self.v_mask,
                               self.mask_sb, self.tau2, self.w, out=out, **({} if self.robust is None else dict(robust=self.robust)))


class _Chamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan, matches, vertex_matches, vis_cache=None):
        if plan.visibility is not None:                                             # the mask of this pass: the plan carries it to the backward pass
            c = vis_cache
            if c is None or c["mask"] is None or c["t"] % c["every"] == 0:
                plan.see(x.detach(), plan.scans.viewpoints)
                if c is not None:
                    c["mask"] = plan.v_mask
            else:
                plan.v_mask, plan.mask_sb = c["mask"], plan.n
            if c is not None:
                c["t"] += 1
        m = plan.search(x, plan.scans, vertex_matches=vertex_matches and matches is not None)
        loss, counts = plan.loss(m, plan.scans)
        ctx.plan = plan
        partner = (m["idx_sm"], m["d2_sm"]) if plan.surface is None else (m["faces"], m["face"], m["d2_surface"], m["uv"])
        ctx.save_for_backward(x, counts, m["idx_ms"], m["d2_ms"], *partner)
        if matches is not None:
            matches.update(m)
        return loss

    @staticmethod
    def backward(ctx, gL):
        x, counts, idx_ms, d2_ms, *partner = ctx.saved_tensors
        p = ctx.plan
        bwd = ops.chamfer_bwd if p.surface is None else ops.chamfer_surface_bwd
        g = bwd(x, p.n, p.scans.points, p.scans.counts, *partner, idx_ms, d2_ms, p.v_mask, p.mask_sb, counts, p.tau2, p.w,
                gL.to(torch.float32).contiguous(), **({} if p.robust is None else dict(robust=p.robust)))
        return g, None, None, None, None


def chamfer(x_hat, scans, n=None, vertex_mask=None, trunc=None, w_model_to_scan=0.0, matches=None, faces=None, normal_angle=None,
            normal_faces=None, gate_on="vertices", visibility=None, visibility_faces=None, grazing_angle=None, robust=None, robust_scale=None):
    """Chamfer distance between decoded bodies and their scans, one value per body [B], differentiable w.r.t. x_hat:

        L[b] = mean_j min(|s_j - nn_x(s_j)|^2, trunc^2)  +  w_model_to_scan * mean_{i active} min(|x_i - nn_s(x_i)|^2, trunc^2)

    x_hat [B, rows, 3] fp32 on the GPU; scans: a ScanBatch (or clouds, packed on the spot) of the same B, in the model's
    normalised frame (no alignment is done here).  n: how many leading rows of x_hat are model vertices.  n=None means
    rows - 1, because every model of this package appends a dummy row to what it decodes; pass n=rows for a bare vertex tensor.
    Rows >= n are never matched and get no gradient - do not slice x_hat instead.  vertex_mask [n] or [B, n]: False = vertex
    takes no part (not a target, no term of its own).  trunc: distances beyond it are cut to it and stop pulling (None: none).
    w_model_to_scan = 0 skips the model -> scan search altogether - the setting for a partial scan.  The gradient flows through
    the nearest indices found in the forward pass; the scan takes none.  matches: a dict that receives what the forward pass
    found (indices, distances, the arguments they belong to) for `pose_update`; None (the default) records nothing.

    faces: None (the default: everything above, bit for bit), or a FaceTable / integer array [nF, 3] of the model's triangles.
    Then the scan -> model term is the squared distance to the closest point of the SURFACE (`nearest_surface`), nn_x(s_j) being
    that point, and its gradient reaches the three corners of the face with the foot point's barycentric weights.  The model ->
    scan term (vertex to scan point), trunc, vertex_mask (a triangle with a masked corner is no target) and n keep their meaning.
    `matches` receives what it receives without faces - the VERTEX matches, which were computed for the search's bound - plus
    `face`, `uv`, `d2_surface` and the table `faces`; `pose_update` works on the vertex pairs unless it is called with
    surface=True, which takes the foot points instead.  Whenever a face table is at hand (`faces`, or `normal_faces` with or
    without a gate) `matches` also receives it as `normal_faces`, a FaceTable (else None) - what `pose_update(..., step="plane")`
    computes the model's normals from - and a gated pass records the normals it has computed as `tn` (else None).

    normal_angle: None (the default: everything above, bit for bit, whether or not the scans carry normals), or an angle in
    degrees in (0, 180].  Then a scan point and a vertex are a pair only when their normals - `scans.normals` and
    `vertex_normals(x_hat)`, computed once per forward pass from `normal_faces` (a FaceTable or an integer array) - differ by at
    most that angle, in both directions (sh_nearest_points_gated; the test is cos(angle) against the fp32 dot product; 180 opens
    the gate and gives the ungated bits).  A zero ("unknown") normal is compatible only for angles >= 90.  A point with no
    compatible partner is recorded as idx -1, d2 +inf and counts as truncated: it adds trunc^2 and takes no part in the
    gradient or in `pose_update` - which is why a gate needs `trunc`.  This gate, on VERTEX normals, is not built together with
    `faces=`.

    gate_on: "vertices" (the default: everything above, bit for bit, every error included) or "surface" - the gate for `faces=`,
    on the FACE's normal (needs faces, normal_angle, scan normals and trunc; normal_faces may be omitted and is then `faces`).
    The scan -> model term is the distance to the closest point of the faces whose normal (`face_normals(x_hat)`, once per
    forward pass) lies within normal_angle of the point's (sh_nearest_surface_gated: exact, bounded by the gated search over the
    face centres); a point with no compatible face is recorded as face -1, d2 +inf and counts as truncated.  The model -> scan
    term stays vertex to scan point and is gated by the vertex normals as above.  The backward pass is that of `faces=`.
    `matches` keeps its keys: `face`, `uv`, `d2_surface` are the gated surface results, `idx_sm` / `d2_sm` the gated VERTEX
    matches (one more gated vertex search, run only when `matches` is given), `tn` the vertex normals when they were computed.
    180 degrees gives the ungated `faces=` loss and gradient, bit for bit.

    visibility: None (the default: everything above, bit for bit, the same launches) or "viewpoint" - for a partial scan taken
    from one sensor position, `scans.viewpoints` (ScanBatch(..., viewpoints=), in the model's frame like the scan).  Only the
    model vertices that sensor sees take part: the mask of this pass is vertex_mask AND `visible_vertices(x_hat, visibility_faces,
    scans.viewpoints, vertex_mask=, grazing_angle=)`, recomputed in every forward pass (sh_vertex_visibility) and read by the
    searches, the loss and the gradient exactly as a given vertex_mask is - the unseen back of the model is no target and has
    no term, so w_model_to_scan > 0 becomes usable on one-view scans.  visibility_faces: the occluding triangles (default:
    faces, else normal_faces; one of the three is needed).  grazing_angle: None, or degrees in (0, 90] - a vertex must also face
    the sensor to within that angle.  A body whose viewpoint row holds a NaN is a full scan: no vertex of it is hidden.  The
    scan's own points are not tested for visibility.

    robust: None (the default - off: everything above, bit for bit, the same launches) or "geman-mcclure" / "huber", with
    robust_scale = sigma > 0 in the model's normalised units (both or neither).  Every term of both directions is then
    rho(min(d2, trunc^2)) instead of min(d2, trunc^2) - Geman-McClure rho = u sigma^2 / (sigma^2 + u), bounded by sigma^2, or
    Huber on the distance, rho = u up to sigma^2 and 2 sigma sqrt(u) - sigma^2 beyond (include/sh_kernels.h, "Robust terms") - and
    a kept pair pulls with w = d rho / d u times its plain gradient (`robust_weights`), the corners of a foot point included.
    Far points - hair, clothing, a floor patch, flying pixels - fade out smoothly instead of dominating or being cut at trunc;
    trunc keeps its meaning (and a gate still needs it).  Works with every other argument.  ValueError for an unknown name, a
    scale without a name, a name without a scale, or a scale that is not a positive finite number."""
    return _chamfer(x_hat, scans, n, vertex_mask, trunc, w_model_to_scan, matches, faces, normal_angle, normal_faces, gate_on,
                    visibility=visibility, visibility_faces=visibility_faces, grazing_angle=grazing_angle, robust=robust,
                    robust_scale=robust_scale)


def _chamfer(x_hat, scans, n, vertex_mask, trunc, w_model_to_scan, matches, faces, normal_angle, normal_faces, gate_on, vertex_matches=True,
             visibility=None, visibility_faces=None, grazing_angle=None, vis_cache=None, robust=None, robust_scale=None):
    """`chamfer`, and what editing.fit_scan / register_scan may add: vertex_matches=False when the pose update will read the foot
    points, so that a face-normal-gated pass skips the vertex search it would run for `matches` alone; vis_cache, a dict
    (every=, t=0, mask=None), makes a pass reuse the last visibility mask unless t is a multiple of `every`."""
    plan = _MatchPlan("chamfer", x_hat, _check_pair(x_hat, scans, n, "chamfer"), vertex_mask, trunc, w_model_to_scan, faces, normal_angle,
                      normal_faces, gate_on, record=matches is not None, visibility=visibility, visibility_faces=visibility_faces,
                      grazing_angle=grazing_angle, robust=robust, robust_scale=robust_scale)
    if visibility is None:
        return _Chamfer.apply(x_hat, plan, matches, vertex_matches)
    return _Chamfer.apply(x_hat, plan, matches, vertex_matches, vis_cache)


# ------------------------------------------------------------------------------------------------ alignment
class Pose:
    """B similarities scan frame -> model frame, s' = A s + t with A = scale * R (R a proper rotation, scale > 0).  One fp32
    buffer `packed` [B, 12] (A row-major, then t - the layout of include/sh_kernels.h) of which `A` [B, 3, 3] and `t` [B, 3] are
    views, plus `scale` [B].  Lives wherever its tensors live; `apply` runs on the GPU only.  `solved` is None except on the pose
    `align(..., step="plane")` returns, where it is int32 [iters, B]: row k tells which bodies' k-th point-to-plane system was
    solved (0: singular, that step left the pose as it was)."""

    solved = None
    visible = None                                                                      # bool [iters, B, n] on the pose `align(..., visibility=)` returns

    def __init__(self, A, t, scale=None):
        A = torch.as_tensor(A, dtype=torch.float32)
        t = torch.as_tensor(t, dtype=torch.float32, device=A.device)
        if A.dim() != 3 or tuple(A.shape[1:]) != (3, 3) or tuple(t.shape) != (A.shape[0], 3):
            raise ValueError("Pose: A must be [B, 3, 3] and t [B, 3], got %s and %s" % (tuple(A.shape), tuple(t.shape)))
        if scale is None:
            scale = torch.linalg.det(A.double().cpu()).abs().pow(1.0 / 3.0)
        scale = torch.as_tensor(scale, dtype=torch.float32).to(A.device).reshape(-1).contiguous()
        if tuple(scale.shape) != (A.shape[0],):
            raise ValueError("Pose: scale must be [%d]" % A.shape[0])
        self.packed = torch.cat([A.reshape(-1, 9), t], 1).contiguous()
        self.scale = scale

    @classmethod
    def from_packed(cls, packed, scale):
        out = cls.__new__(cls)
        out.packed, out.scale = packed, scale
        return out

    @classmethod
    def identity(cls, B, device):
        packed = torch.zeros((int(B), 12), dtype=torch.float32, device=device)
        packed[:, 0] = packed[:, 4] = packed[:, 8] = 1.0
        return cls.from_packed(packed, torch.ones(int(B), dtype=torch.float32, device=device))

    @property
    def A(self):
        return self.packed[:, :9].view(-1, 3, 3)

    @property
    def t(self):
        return self.packed[:, 9:]

    def __len__(self):
        return self.packed.shape[0]

    def clone(self):
        return Pose.from_packed(self.packed.clone(), self.scale.clone())

    def select(self, sl):
        return Pose.from_packed(self.packed[sl].contiguous(), self.scale[sl].contiguous())

    def apply(self, points, counts=None):
        """A p + t for every point, in the one fp32 expression of sh_transform_points.  points: a ScanBatch (-> ScanBatch, rows
        beyond the counts zero; its normals, if any, rotated by R = A / scale through the same kernel) or fp32 HIP points
        [B, M, 3] with optional live counts [B] (-> tensor)."""
        if isinstance(points, ScanBatch):
            nrm = None if points.normals is None else ops.transform_points(points.normals, points.counts, self.rotation_packed())
            return ScanBatch._from_parts(ops.transform_points(points.points, points.counts, self.packed), points.counts, points.host_counts,
                                         points.perm, nrm)
        B = ops._points(points, "scan.Pose.apply")[0]
        return ops.transform_points(points, ops._count_arg(counts, B, points.device), self.packed)

    def rotation_packed(self):
        """The packed pose of the rotation alone, [B, 12]: R = A / scale row-major, t = 0 - what carries a normal."""
        return torch.nn.functional.pad(self.packed[:, :9] / self.scale[:, None], (0, 3))

    def compose(self, first):
        """The pose that applies `first` and then this one (float64 inside, rounded to fp32 once)."""
        A1, A0 = self.A.double(), first.A.double()
        A = torch.matmul(A1, A0)
        t = torch.matmul(A1, first.t.double()[:, :, None])[:, :, 0] + self.t.double()
        return Pose(A.float(), t.float(), (self.scale.double() * first.scale.double()).float())

    def inverse(self):
        """Model frame -> scan frame (float64 adjugate of A, rounded to fp32 once)."""
        a = self.A.double()
        c0 = torch.linalg.cross(a[:, 1], a[:, 2])
        c1 = torch.linalg.cross(a[:, 2], a[:, 0])
        c2 = torch.linalg.cross(a[:, 0], a[:, 1])
        det = (a[:, 0] * c0).sum(-1)
        inv = torch.stack([c0, c1, c2], dim=2) / det[:, None, None]
        t = -(inv * self.t.double()[:, None, :]).sum(-1)
        return Pose(inv.float(), t.float(), (1.0 / self.scale.double()).float())

    def to_scan_frame(self, x_hat):
        """Model-frame points [B, rows, 3] (decoded vertices) carried back into the scan's frame; plain tensor operations."""
        inv = self.inverse()
        return (x_hat[:, :, None, :] * inv.A[:, None, :, :]).sum(-1) + inv.t[:, None, :]


def _check_pair(x, scans, n, what):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise RuntimeError("semantichuman_amd.scan.%s needs fp32 HIP vertices [B, rows, 3] (got %s); there is no CPU path"
                           % (what, getattr(x, "device", type(x))))
    if not isinstance(scans, ScanBatch):
        scans = ScanBatch(scans, x.device)
    B, rows, _ = ops._points(x, "scan." + what)
    ops._points(scans.points, "scan." + what)
    if len(scans) != B:
        raise ValueError("%s: %d bodies, %d scans" % (what, B, len(scans)))
    n = rows - 1 if n is None else int(n)
    if not 0 < n <= rows:
        raise ValueError("%s: n = %d outside (0, %d]" % (what, n, rows))
    return scans, B, rows, n


# ------------------------------------------------------------------------------------------------ free space and silhouette
def _free_space_fwd(x, field, cam, n, v_mask, mask_sb, margin):
    """The forward entry point on a field's planes -> (term, kind, loss, counts).  cam None: one camera, x in its frame."""
    return ops._free_space_fwd(cam is not None, x, n, cam, field.cls, field.z, field.nearest, field.intrinsics, v_mask, mask_sb, margin,
                               rays=field._lens())


class _FreeSpace(torch.autograd.Function):
    """x in the frame cam [B, V, 12] starts from - the model's; cam is its way into every camera's frame, a constant of the step - or,
    cam None, in the one camera's own frame."""

    @staticmethod
    def forward(ctx, x, field, cam, n, v_mask, mask_sb, margin):
        _, _, loss, counts = _free_space_fwd(x, field, cam, n, v_mask, mask_sb, margin)
        ctx.args = (field, n, v_mask, mask_sb, margin)
        ctx.save_for_backward(x, cam, counts)
        return loss

    @staticmethod
    def backward(ctx, gL):
        x, cam, counts = ctx.saved_tensors
        field, n, v_mask, mask_sb, margin = ctx.args
        g = ops._free_space_bwd(cam is not None, x, n, cam, field.cls, field.z, field.nearest, field.intrinsics, v_mask, mask_sb, margin, counts,
                                gL.to(torch.float32).contiguous(), rays=field._lens())
        return g, None, None, None, None, None, None


def free_space_cameras(field, pose=None):
    """The way from the model's frame into every camera of a rig field -> cam fp32 [B, V, 12] = (M | c), q = M x + c
    (sh_free_space_cameras; include/sh_kernels.h, "Free space from a rig"): the inverse of `pose.compose(E_v)` with E_v the
    camera's extrinsic, M = R_v^T A^-1 and c = -R_v^T (A^-1 t + t_v), formed in fp64 and rounded once.  pose: the `Pose` (rig frame
    -> model frame) or None, the identity.  An absent camera, or a body whose A is singular, gives a NaN row: that camera sees no
    vertex.  One launch, nothing synchronised.  What `free_space(..., cameras=)` takes when the pose stays as it is over many
    calls.  ValueError for a field that is no rig field or a pose of another batch size."""
    what = "free_space_cameras"
    if not isinstance(field, DepthField) or field.views is None:
        raise ValueError("%s: the field must be a rig field (DepthField.from_depth(..., extrinsics=))" % what)
    if pose is not None and (not isinstance(pose, Pose) or len(pose) != len(field)):
        raise ValueError("%s: pose must be a scan.Pose of %d bodies" % (what, len(field)))
    return ops.free_space_cameras(field.extrinsics, None if pose is None else pose.packed.contiguous())


def _check_free_space_weights(what, field, B, margin, weights=()):
    """The ValueErrors of the free-space arguments: a DepthField of B images, a margin and weights that are >= 0 (and not NaN)."""
    if not isinstance(field, DepthField):
        raise ValueError("%s: the field must be a scan.DepthField, got %s" % (what, type(field).__name__))
    if len(field) != B:
        raise ValueError("%s: %d bodies, a field of %d images" % (what, B, len(field)))
    if not float(margin) >= 0:
        raise ValueError("%s: the margin must be >= 0, got %r" % (what, margin))
    for name, w in weights:
        if not float(w) >= 0:
            raise ValueError("%s: %s must be >= 0, got %r" % (what, name, w))


def _free_space_args(what, x_hat, field, pose, n, vertex_mask, margin, cameras=None):
    """The checks of `free_space` and `free_space_kinds` -> (x, n, v_mask, mask_sb, cam).  One camera (cam None): x is x_hat in the
    camera's frame (`pose.to_scan_frame`, torch).  A rig field: x is x_hat as it is and cam [B, V, 12] carries it into every
    camera's frame inside the kernels - `cameras` as given, else one `free_space_cameras` launch."""
    if not (torch.is_tensor(x_hat) and x_hat.is_cuda):
        raise RuntimeError("semantichuman_amd.scan.%s needs fp32 HIP vertices [B, rows, 3] (got %s); there is no CPU path"
                           % (what, getattr(x_hat, "device", type(x_hat))))
    B, rows, _ = ops._points(x_hat, "scan." + what)
    _check_free_space_weights(what, field, B, margin)
    if pose is not None and len(pose) != B:
        raise ValueError("%s: %d bodies, %d poses" % (what, B, len(pose)))
    n = rows - 1 if n is None else int(n)
    if not 0 < n <= rows:
        raise ValueError("%s: n = %d outside (0, %d]" % (what, n, rows))
    v_mask, mask_sb = ops._mask_arg(vertex_mask, B, n, x_hat.device)
    if field.views is None:
        if cameras is not None:
            raise ValueError("%s: cameras= goes with a rig field (DepthField.from_depth(..., extrinsics=))" % what)
        return (x_hat if pose is None else pose.to_scan_frame(x_hat)), n, v_mask, mask_sb, None
    if cameras is None:
        cameras = free_space_cameras(field, pose)
    elif not (torch.is_tensor(cameras) and cameras.device == x_hat.device and cameras.dtype == torch.float32
              and tuple(cameras.shape) == (B, field.views, 12)):
        raise ValueError("%s: cameras must be an fp32 tensor [%d, %d, 12] on the device of x_hat (scan.free_space_cameras), got %s"
                         % (what, B, field.views, tuple(getattr(cameras, "shape", ()))))
    return x_hat, n, v_mask, mask_sb, cameras.detach().contiguous()


def free_space(x_hat, field, *, pose=None, n=None, vertex_mask=None, margin=0.0, cameras=None):
    """What a one-view depth image adds to a fit beyond its points: -> (free [B], silhouette [B]), differentiable w.r.t. x_hat
    (sh_free_space_fwd / _bwd; include/sh_kernels.h, "Depth field").  x_hat [B, rows, 3] fp32 on the GPU, field: a `DepthField` of
    the same B.  Every active vertex is projected into its image (the field's intrinsics; its lens, if it has one) and reads the ONE pixel it
    falls into:
      * a SURFACE pixel whose depth, less `margin`, lies behind the vertex: the vertex stands in space the sensor saw through -
        it adds (z - margin - Z)^2 to `free`;
      * an EMPTY pixel: the body does not project here - it adds to `silhouette` the squared offset of the vertex from the ray
        through the nearest pixel that is not EMPTY, at the vertex's own depth (the same units as `free`);
      * an UNKNOWN pixel, a pixel outside the image, a vertex behind the camera: nothing.
    Both are means over the active vertices.  n and vertex_mask as in `chamfer` (n=None: rows - 1).  pose: None - x_hat is in the
    camera's frame - or a `Pose` (scan frame -> model frame): the vertices are carried into the camera's frame by
    `pose.to_scan_frame` (plain torch, differentiable) and both values multiplied by pose.scale^2, which puts them in the units
    of x_hat, where they add to a Chamfer value.  The pose takes no gradient.
    Limits: nearest-pixel sampling - the image is read as a constant, the nearest pixel too, so there is no image gradient and
    the value steps as a vertex crosses a pixel boundary; no robust or truncated form.  A field made with distortion= (`field.rays`)
    is read through its lens model - the rational model of "Camera rays", no fisheye or equidistant model: the vertex is projected
    by the forward model, a vertex beyond the fold-back limit is outside, the silhouette ray comes from the table (a pixel without
    a ray: no term), and the gradient needs no Jacobian of the lens (sh_free_space_views_rays_fwd / _bwd).
    A RIG field (`DepthField.from_depth(..., extrinsics=)`; a rig of one serves a single camera): every vertex is judged by each
    of the V cameras in turn and both values are sums over the cameras of the per-camera means (sh_free_space_views_fwd / _bwd;
    "Free space from a rig").  x_hat stays in the model's frame: `pose` is then the Pose rig frame -> model frame (None: the
    model's frame is the rig's), and the way into every camera's frame - the inverse of `pose.compose(E_v)` - is one small launch
    (`free_space_cameras`) whose result the two kernels apply themselves; no torch launches for the transform.  cameras: that
    result [B, V, 12], computed by the caller once while the pose stays as it is (`pose` is still read for its scale).  One
    resolution per rig; an absent camera sees nothing.
    ValueError for a field of another batch size, a negative margin, or cameras of the wrong shape or without a rig field."""
    x, n, v_mask, mask_sb, cam = _free_space_args("free_space", x_hat, field, pose, n, vertex_mask, margin, cameras)
    loss = _FreeSpace.apply(x, field, cam, n, v_mask, mask_sb, float(margin))
    if pose is not None:
        loss = loss * (pose.scale * pose.scale)[:, None]
    return loss[:, 0], loss[:, 1]


def free_space_kinds(x_hat, field, *, pose=None, n=None, vertex_mask=None, margin=0.0, cameras=None):
    """What `free_space` did with every vertex -> (kind uint8 [B, n]: 0 no term, 1 free space, 2 silhouette, 3 an UNKNOWN pixel,
    4 outside the image or behind the camera; counts int32 [B, 4] = active vertices and how many of kind 1, 2 and 4).  A rig
    field: kind [B, V, n] and counts [B, V, 4], per camera.  Not differentiable."""
    x, n, v_mask, mask_sb, cam = _free_space_args("free_space_kinds", x_hat.detach() if torch.is_tensor(x_hat) else x_hat, field, pose, n,
                                                  vertex_mask, margin, cameras)
    _, kind, _, counts = _free_space_fwd(x, field, cam, n, v_mask, mask_sb, float(margin))
    return kind, counts


def moment_pose(scans, x, n=None, vertex_mask=None, scale=True):
    """The start pose that needs no matches: the scan's centroid onto the centroid of the (unmasked) model vertices and, with
    scale=True, its RMS radius onto theirs; the rotation is the identity.  x [B, rows, 3] on the GPU, n / vertex_mask as in
    `chamfer`.  A one-off in torch (float64 sums), outside every loop."""
    scans, B, rows, n = _check_pair(x, scans, n, "moment_pose")
    v_mask, _ = ops._mask_arg(vertex_mask, B, n, x.device)
    s = scans.points.double()
    ws = (torch.arange(s.shape[1], device=x.device)[None, :] < scans.counts[:, None]).double()
    wx = torch.ones((B, n), dtype=torch.float64, device=x.device) if v_mask is None else v_mask.double().expand(B, n)
    xv = x.detach()[:, :n].double()

    def stats(p, w):
        tot = w.sum(1).clamp_min(1.0)
        c = (p * w[:, :, None]).sum(1) / tot[:, None]
        r2 = (((p - c[:, None, :]) ** 2).sum(-1) * w).sum(1) / tot
        return c, r2

    cs, rs = stats(s, ws)
    cx, rx = stats(xv, wx)
    c = torch.sqrt(rx / rs) if scale else torch.ones_like(rs)
    c = torch.where(torch.isfinite(c) & (c > 0), c, torch.ones_like(c))
    A = torch.eye(3, dtype=torch.float64, device=x.device)[None] * c[:, None, None]
    return Pose(A.float(), (cx - c[:, None] * cs).float(), c.float())


def _plane_normals(what, m, surface):
    """The vertex normals a point-to-plane step on the matches m reads: None when it reads none (surface form, scan -> model only),
    m["tn"] when the matches carry them, else computed from the FaceTable m["normal_faces"] (one sh_vertex_normals)."""
    if surface and not m["w_ms"] > 0.0:
        return None
    tn = m.get("tn")
    if tn is None:
        ft = m.get("normal_faces")
        if not isinstance(ft, FaceTable):
            raise ValueError("%s: step='plane' needs the model's normals - matches recorded with a face table (faces= or normal_faces=), or a "
                             "'normal_faces' FaceTable / 'tn' entry put into them" % what)
        if ft.n != m["n"]:
            raise ValueError("%s: the face table was made for %d vertices, the model has %d" % (what, ft.n, m["n"]))
        tn = ops.vertex_normals(m["x"], ft.faces, ft.vf_ptr, ft.vf_idx, ft.n)
    return tn


def pose_update(pose, scans, aligned, matches, mode="similarity", partials=None, surface=False, step="point", solved=None, robust=None,
                robust_scale=None):
    """One closed-form pose step from recorded matches, no search: moments of the matched pairs (`matches`, as `chamfer(...,
    matches=)` or `align` fill it, found on `aligned`), the pose increment that minimises the same weighted squared distances,
    composed into `pose` in place, and `aligned.points` overwritten with the ORIGINAL `scans` under the new pose.  Three
    launches; when both batches carry normals, `aligned.normals` is overwritten with the ORIGINAL normals under the new pose's
    rotation (one more sh_transform_points).  surface=True: the scan -> model partner of a scan point is its foot point on the
    model's surface (`face`, `uv`, `d2_surface` and `faces` of the matches, as `chamfer(..., faces=, matches=)` or
    `align(..., faces=)` record them) instead of its nearest vertex - the step then lowers the surface Chamfer value; still three
    launches.  ValueError if the matches carry no surface result.

    step: "point" (the default: everything above, bit for bit) or "plane" - the linearised point-to-plane step on the same pairs
    (sh_align_plane_moments / _surface, sh_align_plane_solve): the residual of a pair is measured along the model's normal at the
    partner (the recorded face's normal for a foot point, the vertex normal otherwise), and the increment solves the 3 / 6 / 7
    normal equations of `mode`.  Still three launches, plus one sh_vertex_normals when vertex normals are read (vertex form, or
    w_model_to_scan > 0) and the matches carry none as `tn`; they are then computed from the matches' `normal_faces` FaceTable
    (recorded by `chamfer` whenever it was given faces= or normal_faces=).  The step is Gauss-Newton: it minimises the linearised
    residual, so the Chamfer value is not guaranteed to fall.  solved: None, or an int32 HIP tensor [B] that receives 1 per body
    whose system was solved and 0 where it was singular to working precision (no pairs, too few, planar or parallel normals) -
    that body's pose is left exactly as it was.  ValueError when the normals are needed and cannot be had.

    When `aligned` carries viewpoints (the batch `align(..., visibility="viewpoint")` returns does; `Pose.apply` gives none), they
    are overwritten with the ORIGINAL `scans.viewpoints` under the new pose - the sensor moves with its scan (one more
    sh_transform_points over [B, 1, 3]).

    robust / robust_scale: None (the default: everything above, bit for bit, the same launches) or the robust term of `chamfer` -
    one IRLS step: every kept pair enters the moments (or the normal equations of step="plane") with the weight
    `robust_weights` gives the distance recorded for it, so the increment minimises the weighted squared distances; the solve is
    unchanged (sh_align_moments_robust and its three twins).  Pass what the matches were recorded with.  ValueError as in
    `chamfer`."""
    m = matches
    rb = _robust_arg("pose_update", robust, robust_scale)
    if step not in ("point", "plane"):
        raise ValueError("pose_update: step must be 'point' or 'plane'")
    if surface and any(m.get(k) is None for k in ("face", "uv", "d2_surface", "faces")):
        raise ValueError("pose_update: surface=True needs the matches of a surface search (chamfer(..., faces=, matches=) or "
                         "align(..., faces=)); these carry none")
    plane = step == "plane"
    normals = (_plane_normals("pose_update", m, surface),) if plane else ()
    partner = (m["faces"], m["face"], m["uv"], m["d2_surface"]) if surface else (m["idx_sm"], m["d2_sm"])
    moments = ((ops.align_moments, ops.align_moments_surface), (ops.align_plane_moments, ops.align_plane_moments_surface))[plane][bool(surface)]
    part = moments(aligned.points, scans.counts, m["x"], m["n"], m["v_mask"], m["mask_sb"], *normals, *partner, m["idx_ms"], m["d2_ms"], m["tau2"],
                   m["w_ms"], out=partials, **({} if rb is None else dict(robust=rb)))
    solve = (aligned.points.shape[1], m["n"], scans.counts, m["w_ms"], mode, pose.packed, pose.scale, pose.packed, pose.scale)
    if plane:
        ops.align_plane_solve(part, *solve, solved=solved)
    else:
        ops.align_solve(part, *solve)
    ops.transform_points(scans.points, scans.counts, pose.packed, out=aligned.points)
    if scans.normals is not None and aligned.normals is not None:
        ops.transform_points(scans.normals, scans.counts, pose.rotation_packed(), out=aligned.normals)
    if scans.viewpoints is not None and aligned.viewpoints is not None:                 # only `align(..., visibility=)` gives `aligned` any
        _move_viewpoints(scans.viewpoints, pose.packed, out=aligned.viewpoints)
    return part


def align(x, scans, mode="similarity", iters=30, init="moments", trunc=None, w_model_to_scan=1.0, n=None, vertex_mask=None, chunks=0,
          normal_angle=None, normal_faces=None, faces=None, cull=True, step="point", gate_on="vertices", visibility=None,
          visibility_faces=None, grazing_angle=None, robust=None, robust_scale=None):
    """Batched ICP: the pose (scan frame -> model frame) that brings each scan onto its body x[b], by alternating the
    nearest-point search with the closed-form pose of the matched pairs.  Pairs and weights are those of `chamfer` with the same
    trunc / w_model_to_scan / n / vertex_mask, so every iteration lowers that Chamfer value (up to fp32 rounding).

    mode: "translation", "rigid" or "similarity".  init: "moments" (`moment_pose`; without scale unless mode is "similarity"),
    "identity", or a Pose.  Per iteration: the ORIGINAL scan under the pose so far -> search -> the logged Chamfer value ->
    moments -> solve; rounding therefore does not build up in the points.  No host synchronisation.  chunks: the search's split
    (every value gives the same bits).  Returns (pose, the aligned scans as a ScanBatch, chamfer [iters, B] - row k is the value
    BEFORE the k-th update).  Not differentiable.  normal_angle / normal_faces: the normal gate of `chamfer` on both searches of
    every iteration (None: none, the same bits as ever); the model's normals are computed once, the scan's are carried by the
    pose's rotation from the ORIGINAL normals each iteration.  Needs scans.normals, normal_faces and trunc.

    faces: None (the default: everything above, bit for bit), or the model's triangles (a FaceTable or an integer array [nF, 3]) -
    point-to-surface ICP.  The scan -> model partner of a scan point is then the closest point of the SURFACE, the pairs and
    weights are those of `chamfer(..., faces=)`, and it is that surface Chamfer value that the log holds and that every iteration
    lowers.  Per iteration: the vertex search (its distance bounds the surface search; recorded as ever), `nearest_surface` into
    buffers allocated once, the model -> scan search if w_model_to_scan > 0 (vertex to scan point, unchanged), the logged value,
    then the surface moments (sh_align_moments_surface), the solve and the transform.  The face table is built once.  cull=False
    makes the surface search test every (point, triangle) pair - same bits, many times the work.  A scan packed with
    order="morton" makes the culled search cheaper.

    Limits.  ICP is local: the moment start fixes translation and scale, not rotation - a scan rotated by more than about 45
    degrees against the model needs a caller-supplied start pose (no principal-axes or multi-start search here).  mode
    "similarity" with w_model_to_scan = 0 and init="identity" can shrink the scan into the model; the defaults avoid it.
    Partial scans: mode="rigid", w_model_to_scan=0.  A similarity reaches the model's frame only under the normalisations that
    are similarities (zeromean, zeroroot, onelength, small), not under gass or normal.  With faces= the closed form is still
    point-to-point (on foot points): along the surface it slides slowly - step="plane" is the remedy.  faces= together
    with normal_angle needs gate_on="surface" (the gate on vertex normals is not built for the surface distance), and the model
    -> scan term stays vertex to scan point.

    gate_on: "vertices" (the default: everything above, bit for bit) or "surface" - with faces=, normal_angle, scan normals and
    trunc: every iteration's surface search is the face-normal-gated one of `chamfer(..., gate_on="surface")` (face normals
    once, x is fixed; the scan's normals follow the pose), no vertex search is run for the scan -> model side, and the model ->
    scan search is gated by the vertex normals.  Works with step="point" and step="plane".

    step: "point" (the default: everything above, bit for bit) or "plane" - every iteration's pose step is the linearised
    point-to-plane step of `pose_update(..., step="plane")` on the same pairs: a scan point may slide along the model's surface
    and is pulled along the normal only.  On noise-free surface samples of the 170-vertex model, float64, it is within 1e-3 of the
    extent after 3 to 5 iterations where the closed form needs more than 20 (tests/align_plane_ref.py).  The model's vertex
    normals are needed in vertex form and whenever w_model_to_scan > 0; x is fixed, so they are computed once before the loop
    (shared with the gate's when normal_angle is given) from `faces`, or in vertex form from `normal_faces` - ValueError when
    neither is given.  The step is Gauss-Newton, without damping or line search: the logged value is not guaranteed to fall.  The
    returned pose carries `solved`, int32 [iters, B]: 0 where a body's system was singular to working precision (no kept pair, too
    few, planar or parallel normals) - that iteration left that body's pose exactly as it was.

    visibility: None (the default: everything above, bit for bit, the same launches) or "viewpoint" - the partial-scan form of
    `chamfer(..., visibility=)`, with visibility_faces / grazing_angle as there.  `scans.viewpoints` live in the SCAN's frame and
    move with the pose: every iteration carries the original viewpoint through the pose so far (the sh_transform_points call
    that moves the scan, on [B, 1, 3]) and recomputes the mask - x is fixed, the sensor moves - before the searches.  The returned
    batch carries the viewpoints in the model's frame, and the returned pose carries `visible`, bool [iters, B, n]: row k is the
    mask iteration k used.  With it w_model_to_scan = 1 works on one-view scans: the unseen side of the model pulls nothing.
    The start pose `init="moments"` still takes the centroid and radius of the whole model.

    robust / robust_scale: None (the default - off: everything above, bit for bit, the same launches) or the robust term of
    `chamfer` ("geman-mcclure" / "huber" with sigma): ICP becomes iteratively re-weighted least squares.  The logged value is the
    robust Chamfer value, and every pose step weighs a kept pair by `robust_weights` of the distance this iteration's search
    recorded for it (`pose_update(..., robust=)`), with step="point" and step="plane", vertex and surface partners alike.  Scan
    points with no counterpart on the model - a floor patch, a hand-held object - then stop biasing the pose without a trunc
    tight enough to cut them.  sigma is fixed for the run (no annealing: run twice for a coarse and a fine pass); the start pose
    `init="moments"` is not robust - it still takes the centroid and radius of the whole scan."""
    pair = _check_pair(x, scans, n, "align")
    if mode not in ops.ALIGN_MODES:
        raise ValueError("align: mode must be one of %s" % sorted(ops.ALIGN_MODES))
    iters = int(iters)
    if iters < 0:
        raise ValueError("align: iters must be >= 0")
    x = x.detach()
    plan = _MatchPlan("align", x, pair, vertex_mask, trunc, w_model_to_scan, faces, normal_angle, normal_faces, gate_on, step,
                      visibility=visibility, visibility_faces=visibility_faces, grazing_angle=grazing_angle, robust=robust, robust_scale=robust_scale)
    rb = {} if plan.robust is None else dict(robust=robust, robust_scale=robust_scale)
    scans, B, rows, n = pair
    w, dev = plan.w, x.device
    if isinstance(init, Pose):
        if len(init) != B:
            raise ValueError("align: %d bodies, start pose for %d" % (B, len(init)))
        pose = Pose.from_packed(init.packed.to(dev).contiguous().clone(), init.scale.to(dev).contiguous().clone())
    elif init == "moments":
        pose = moment_pose(scans, x, n, vertex_mask, scale=(mode == "similarity"))
    elif init == "identity":
        pose = Pose.identity(B, dev)
    else:
        raise ValueError("align: init must be 'moments', 'identity' or a Pose")
    aligned = pose.apply(scans)
    log = torch.empty((iters, B), dtype=torch.float32, device=dev)
    M = scans.points.shape[1]

    def pair_buffers(width):
        return torch.empty((B, width), dtype=torch.int32, device=dev), torch.empty((B, width), dtype=torch.float32, device=dev)

    sm = None if plan.kind == SURFACE_GATED else pair_buffers(M)                        # gated surface: no vertex search on the scan -> model side
    ms = pair_buffers(rows) if w > 0.0 else None
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    sf = None if plan.surface is None else (*pair_buffers(M), torch.empty((B, M, 2), dtype=torch.float32, device=dev))
    part = None
    tn = qn = fn = None                                                                 # x is fixed: the model's normals once
    if plan.normals is not None and iters > 0 and not (plan.kind == SURFACE_GATED and w == 0.0):
        tn = ops.vertex_normals(x, plan.normals.faces, plan.normals.vf_ptr, plan.normals.vf_idx, n)
        qn = _query_normals(tn, rows) if plan.cos_min is not None and w > 0.0 else None
    if plan.kind == SURFACE_GATED and iters > 0:
        fn = ops.face_normals(x, plan.surface.faces, n)
    solved = None
    if step == "plane":
        solved = pose.solved = torch.empty((iters, B), dtype=torch.int32, device=dev)
    visible = None
    if plan.visibility is not None:
        aligned.viewpoints = _move_viewpoints(scans.viewpoints, pose.packed)
        visible = torch.empty((iters, B, n), dtype=torch.uint8, device=dev)
        pose.visible = visible.view(torch.bool)
    for k in range(iters):
        if visible is not None:
            plan.see(x, aligned.viewpoints, out=visible[k], static_x=True)
        m = plan.search(x, aligned, (tn, qn, fn), (sm, sf, ms), chunks, cull, vertex_matches=False)
        plan.loss(m, scans, out=(log[k], counts))
        part = pose_update(pose, scans, aligned, m, mode, partials=part, surface=plan.surface is not None, step=step,
                           solved=None if solved is None else solved[k], **rb)
    return pose, aligned, log
