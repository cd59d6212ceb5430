"""Body measurements: bone lengths and girths.

Mirrors reference utils_SH.py:86-161:
  * `cal_length(kps, skl_list)`            utils_SH.py:86-98   -> HIP kernel sh_bone_length
  * `measure_body_quick(v, kps, skl_list, factor_list, edge_point_index_list)`
                                           utils_SH.py:144-161 -> HIP kernels sh_measure_girth + sh_bone_length
  * `measure_body_batch(...)`              the same for a whole batch of meshes in two launches (what
                                           obj2npy.py:93-110 does one mesh at a time in numpy)
  * `cal_girth(face_point, face_normal, points)`  utils_SH.py:100-142, the CALIBRATION step that turns a
    cutting plane into an ordered ring of edge points.  It runs once per template, on the host (float64
    closed form of the reference's 3x3 solves), and its result is packed into `GirthRings`.
The measuring itself has no CPU path: tensors must live on the GPU.

Differentiable forms (new names; the functions above stay forward-only):
  * `girths(v, rings)`        -> sh_measure_girth / sh_measure_girth_bwd
  * `bone_lengths(kps, bones)` -> sh_bone_length / sh_bone_length_bwd
  * `joints(x, J)`            -> sh_joint_regress / sh_joint_regress_bwd   (kps = J @ x[:, :N])
Their backward kernels gather over transposed lists built on the host once (GirthRings, Bones): deterministic, no atomics.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops


class GirthRings:
    """Device tables of P girth rings: CSR over rings of (vertex a, vertex b, factor) edge points
    (the reference keeps them as two pickled lists, cfg.PATH.factor_list / edge_point_index_list)."""

    def __init__(self, factor_list, edge_point_index_list, device):
        assert len(factor_list) == len(edge_point_index_list)
        ptr, a, b, f = [0], [], [], []
        for fac, epi in zip(factor_list, edge_point_index_list):
            epi = np.asarray(epi, dtype=np.int64).reshape(-1, 2)
            fac = np.broadcast_to(np.asarray(fac, dtype=np.float32).reshape(-1), (epi.shape[0],))   # scalar or [n, 1]
            a.append(epi[:, 0]); b.append(epi[:, 1]); f.append(fac)
            ptr.append(ptr[-1] + epi.shape[0])
        self.n_rings = len(factor_list)
        self.max_vertex = int(max(max(x.max() for x in a), max(x.max() for x in b))) if ptr[-1] else -1
        dev = torch.device(device)
        self.ptr = torch.tensor(ptr, dtype=torch.int32, device=dev)
        self.a = torch.from_numpy(np.concatenate(a).astype(np.int32)).to(dev)
        self.b = torch.from_numpy(np.concatenate(b).astype(np.int32)).to(dev)
        self.f = torch.from_numpy(np.concatenate(f).astype(np.float32)).to(dev)
        # transposed lists for the gradient: ring of every ring point, and per vertex row (rows <= max_vertex) the CSR of
        # (ring point, weight) - 1 - f for the point's vertex a, f for its vertex b; a row's entries ordered by point, a before b
        pa = np.concatenate(a).astype(np.int64) if ptr[-1] else np.zeros(0, np.int64)
        pb = np.concatenate(b).astype(np.int64) if ptr[-1] else np.zeros(0, np.int64)
        pf = np.concatenate(f).astype(np.float32) if ptr[-1] else np.zeros(0, np.float32)
        self.n_points = int(ptr[-1])
        pt_ring = np.repeat(np.arange(self.n_rings, dtype=np.int32), np.diff(np.asarray(ptr)))
        self.vt_rows = self.max_vertex + 1
        vt_ptr, vt_pt, vt_w = transpose_lists(
            np.concatenate([pa, pb]), np.concatenate([np.arange(self.n_points), np.arange(self.n_points)]),
            np.concatenate([np.float32(1) - pf, pf]), np.concatenate([np.zeros(self.n_points, np.int64), np.ones(self.n_points, np.int64)]),
            self.vt_rows)
        self.pt_ring = torch.from_numpy(pt_ring).to(dev)
        self.vt_ptr = torch.from_numpy(vt_ptr).to(dev)
        self.vt_pt = torch.from_numpy(vt_pt).to(dev)
        self.vt_w = torch.from_numpy(vt_w).to(dev)

    def tables(self):
        return self.ptr, self.a, self.b, self.f

    def transposed(self):
        """(pt_ring, vt_ptr, vt_pt, vt_w, rows covered) - the lists sh_measure_girth_bwd gathers over."""
        return self.pt_ring, self.vt_ptr, self.vt_pt, self.vt_w, self.vt_rows


def transpose_lists(row, item, weight, minor, n_rows):
    """Entries (row, item, weight) -> CSR over rows [0, n_rows): (ptr int32 [n_rows + 1], item int32, weight float32), the entries
    of a row ordered by (item, minor) - the fixed order in which the backward kernels sum them."""
    row, item, minor = (np.asarray(t, dtype=np.int64) for t in (row, item, minor))
    weight = np.asarray(weight, dtype=np.float32)
    order = np.lexsort((minor, item, row))
    ptr = np.zeros(n_rows + 1, dtype=np.int32)
    np.cumsum(np.bincount(row, minlength=n_rows)[:n_rows], out=ptr[1:])
    return ptr, item[order].astype(np.int32), weight[order]


def bone_table(skl_list, device):
    """[[a, b] | [a, b, c], ...] -> int32 [P, 3] with -1 for the missing third joint."""
    t = np.full((len(skl_list), 3), -1, dtype=np.int32)
    for i, s in enumerate(skl_list):
        if len(s) not in (2, 3):
            raise ValueError("bone %d: expected 2 or 3 joint ids, got %r" % (i, s))
        t[i, :len(s)] = s
    return torch.from_numpy(t).to(device)


class Bones:
    """A bone list on the device: the forward table of bone_table() and the transposed list of its gradient - per joint
    (rows <= the largest joint id) the CSR of (bone, signed weight): +1 head, -1 tail of a 2-joint bone, -1/2 each tail joint of
    a 3-joint bone; a joint's entries ordered by bone."""

    def __init__(self, skl_list, device):
        self.table = bone_table(skl_list, device)
        t = np.full((len(skl_list), 3), -1, dtype=np.int64)
        for i, sk in enumerate(skl_list):
            t[i, :len(sk)] = sk
        self.n_bones = t.shape[0]
        self.jt_rows = int(t.max()) + 1 if t.size else 0
        bone = np.arange(self.n_bones)
        three = t[:, 2] >= 0
        row = np.concatenate([t[:, 0], t[:, 1], t[three, 2]])
        item = np.concatenate([bone, bone, bone[three]])
        w = np.concatenate([np.ones(self.n_bones), np.where(three, -0.5, -1.0), np.full(int(three.sum()), -0.5)])
        minor = np.concatenate([np.zeros(self.n_bones), np.ones(self.n_bones), np.full(int(three.sum()), 2)])
        ptr, jb, jw = transpose_lists(row, item, w, minor, self.jt_rows)
        dev = torch.device(device)
        self.jt_ptr, self.jt_bone, self.jt_w = (torch.from_numpy(x).to(dev) for x in (ptr, jb, jw))

    def transposed(self):
        return self.jt_ptr, self.jt_bone, self.jt_w, self.jt_rows


def measure_body_batch(v, kps, rings: GirthRings, bones):
    """v [B, rows, 3], kps [B, K, 3], bones = bone_table(...) -> (girth [B, P], length [B, P2])."""
    if rings.max_vertex >= v.shape[1]:
        raise IndexError("girth ring refers to vertex %d but meshes have %d rows" % (rings.max_vertex, v.shape[1]))
    if int(bones.max()) >= kps.shape[1]:
        raise IndexError("bone refers to joint %d but there are %d joints" % (int(bones.max()), kps.shape[1]))
    return ops.measure_girth(v, rings.tables()), ops.bone_length(kps.contiguous(), bones)


def cal_length(kps, skl_list):
    """utils_SH.py:86-98: kps [N_kps, 3] -> length [N_part]."""
    return ops.bone_length(kps[None].contiguous(), bone_table(skl_list, kps.device))[0]


def measure_body_quick(v, kps, skl_list, factor_list, edge_point_index_list):
    """utils_SH.py:144-161: one mesh v [N_v, 3], joints kps [N_kps, 3] -> (girth [N_part], length [N_part])."""
    rings = GirthRings(factor_list, edge_point_index_list, v.device)
    g, l = measure_body_batch(v[None].contiguous(), kps[None], rings, bone_table(skl_list, v.device))
    return g[0], l[0]


# ------------------------------------------------------------------------------------------------ calibration
def cal_girth(face_point, face_normal, points):
    """utils_SH.py:100-142 on the host.  points [N, 2, 3]: end points of the N mesh edges cut by the plane
    through `face_point` with normal `face_normal`.  Returns (girth, X [N, 3], order [N]).

    The reference solves, per edge, the 3x3 system {n.X = n.p ; X lies on the edge's line} with
    torch.linalg.solve; the closed form is  X = a + t d,  d = a - b (zeros replaced by 1e-6 as at :111),
    t = n.(p - a) / n.d.  The ring order is the reference's: sort by the signed angle (degrees) between
    X_0 - mean and X_i - mean, the sign taken from the product of the cross product's components (:131-133).
    """
    p = np.asarray(face_point, dtype=np.float64).reshape(3)
    n = np.asarray(face_normal, dtype=np.float64).reshape(3)
    pts = np.asarray(points, dtype=np.float64)
    a = pts[:, 0, :]
    d = pts[:, 0, :] - pts[:, 1, :]
    d = np.where(d == 0, 1e-6, d)
    t = ((p - a) @ n) / (d @ n)
    X = a + t[:, None] * d
    Xv = X - X.mean(axis=0)
    m = np.sqrt((Xv * Xv).sum(axis=1))
    cos = (Xv[0:1] * Xv[1:]).sum(axis=1) / (m[1:] * m[0])
    theta = np.arccos(cos) / math.pi * 180
    cr = np.cross(np.repeat(Xv[0:1], Xv.shape[0] - 1, axis=0), Xv[1:])
    flag = np.where(cr[:, 0] * cr[:, 1] * cr[:, 2] > 0, 1.0, -1.0)
    order = np.argsort(np.concatenate(([0.0], theta * flag)), kind="stable")
    Xo = X[order]
    girth = np.sqrt(((Xo[0] - Xo[-1]) ** 2).sum()) + np.sqrt(((Xo[:-1] - Xo[1:]) ** 2).sum(axis=1)).sum()
    return float(girth), X, order


def ring_from_plane(v, edges, face_point, face_normal, vert_mask=None):
    """Calibrate one girth ring on a template: the edges of `edges` [E, 2] (optionally only those with both
    ends in `vert_mask`) that straddle the plane, ordered by cal_girth, as (factor [n], edge_point_index [n, 2])
    in the format measure_body_quick consumes (point = v[a] * (1 - factor) + v[b] * factor)."""
    v = np.asarray(v, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.int64)
    side = (v - np.asarray(face_point, dtype=np.float64)) @ np.asarray(face_normal, dtype=np.float64)
    cut = side[edges[:, 0]] * side[edges[:, 1]] < 0
    if vert_mask is not None:
        cut &= vert_mask[edges[:, 0]] & vert_mask[edges[:, 1]]
    e = edges[cut]
    if e.shape[0] < 3:
        raise ValueError("plane cuts %d edges; a ring needs at least 3" % e.shape[0])
    _, X, order = cal_girth(face_point, face_normal, v[e])
    a, b = v[e[:, 0]], v[e[:, 1]]
    fac = np.linalg.norm(X - a, axis=1) / np.linalg.norm(b - a, axis=1)
    return fac[order].astype(np.float32), e[order]


# ------------------------------------------------------------------------------------------------ differentiable forms
class _Girths(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, rings):
        out = ops.measure_girth(v, rings.tables())
        ctx.rings = rings
        ctx.save_for_backward(v)
        return out

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return ops.measure_girth_bwd(v, ctx.rings, g.contiguous()), None


class _BoneLengths(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kps, bones):
        out = ops.bone_length(kps, bones.table)
        ctx.bones = bones
        ctx.save_for_backward(kps)
        return out

    @staticmethod
    def backward(ctx, g):
        (kps,) = ctx.saved_tensors
        return ops.bone_length_bwd(kps, ctx.bones, g.contiguous()), None


class _Joints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, J):
        from .part_losses import joint_regress
        ctx.rows = x.shape[1]
        ctx.save_for_backward(J)
        return joint_regress(x, J)

    @staticmethod
    def backward(ctx, g):
        (J,) = ctx.saved_tensors
        return ops.joint_regress_bwd(g.contiguous(), J, ctx.rows), None


def girths(v, rings: GirthRings):
    """Differentiable girths: v [B, rows, 3] fp32 on the GPU (rows may include the dummy row) -> [B, P].  The gradient w.r.t. v is
    0 on rows no ring touches; a zero-length segment contributes 0."""
    if rings.max_vertex >= v.shape[1]:
        raise IndexError("girth ring refers to vertex %d but meshes have %d rows" % (rings.max_vertex, v.shape[1]))
    return _Girths.apply(v, rings)


def bone_lengths(kps, bones):
    """Differentiable bone lengths: kps [B, K, 3] fp32 contiguous on the GPU; bones a Bones (or a bone list, converted on the
    host) -> [B, P].  A zero-length bone has gradient 0."""
    if not isinstance(bones, Bones):
        bones = Bones(bones, kps.device)
    if bones.jt_rows > kps.shape[1]:
        raise IndexError("bone refers to joint %d but there are %d joints" % (bones.jt_rows - 1, kps.shape[1]))
    return _BoneLengths.apply(kps, bones)


def joints(x, J):
    """Differentiable joint regression kps = J @ x[:, :N]: x [B, rows >= N, 3] fp32 on the GPU, J [K, N] fp32 on the GPU ->
    [B, K, 3].  The gradient of rows >= N (the dummy row) is 0.  J takes no gradient."""
    return _Joints.apply(x, J)
