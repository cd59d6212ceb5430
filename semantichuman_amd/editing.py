"""Inference / editing front-end: the latent and skeleton edits of reference demo.py:64-113
and utils_SH.edit_skl (:412-440) as functions, plus the OBJ writer the demo uses (utils_SH.save_obj :163-195).

All edits are small tensor manipulations on latents / joints; the heavy part is `model.decode`, which runs the
HIP decoder stack.  `decode_edits` reproduces the demo's seven decodes for a (shape, skeleton, style) triple.

Measurement-targeted editing: `fit_latents` optimises part latents through the frozen decoder against any per-body objective
(the decoder's backward pass then computes no weight gradient); `fit_part_girths` asks for girths ("chest +4 %, waist unchanged")
through the differentiable measurements of measure.py; `fit_scan` fits the latents to unregistered point clouds (scans, depth
clouds, meshes of another topology) with the Chamfer objective of scan.py; `register_scan` does the same for scans that arrive
in their own frame and units, solving for the pose (scan.align) before and during the fit.  Both take the free-space and
silhouette terms of a depth image (`free_space=`, a scan.DepthField) on top of the Chamfer objective.
"""
from __future__ import annotations

import numpy as np
import torch

from . import constants, measure, optim, scan
from .part_losses import kps2skl, skl2kps

# utils_SH.py:21-24 (SMPL-style kinematic tree of the 24 body joints)
PARENT = {1: 0, 2: 0, 3: 0, 4: 1, 5: 2, 6: 3, 7: 4, 8: 5, 9: 6, 10: 7, 11: 8, 12: 9, 13: 9, 14: 9, 15: 12, 16: 13, 17: 14,
          18: 16, 19: 17, 20: 18, 21: 19, 22: 20, 23: 21}
CHILDREN = {0: [1, 2, 3], 1: [4], 2: [5], 3: [6], 4: [7], 5: [8], 6: [9], 7: [10], 8: [11], 9: [12, 13, 14], 12: [15], 13: [16],
            14: [17], 16: [18], 17: [19], 18: [20], 19: [21], 20: [22], 21: [23]}


def edit_skl(kps, kps_index, edit_length):
    """utils_SH.py:412-440: scale the bone parent(kps_index) -> kps_index by `edit_length` [N] and move the whole
    sub-tree below the joint along with it.  kps [N, K, 3] -> new kps."""
    parent = kps[:, PARENT[kps_index], :]
    direction = kps[:, kps_index, :] - parent
    shift = direction * (torch.as_tensor(edit_length, dtype=kps.dtype, device=kps.device) - 1)[:, None]
    subtree, stack = [], [kps_index]
    while stack:
        i = stack.pop()
        subtree.append(i)
        stack.extend(CHILDREN.get(i, []))
    new = kps.clone()
    new[:, subtree, :] = new[:, subtree, :] + shift[:, None, :]
    return new


def edit_bone_orientation(skl, target_skl, bone_indices):
    """demo.py:79-81: take the unit directions of the chosen bones from another skeleton ('ori_m' layout [N, n_bones, 4])."""
    out = skl.clone()
    out[:, bone_indices, :3] = target_skl[:, bone_indices, :3]
    return out


def edit_bone_length(skl, bone_indices, factor):
    """demo.py:83-86: scale the lengths (4th component of the 'ori_m' layout) of the chosen bones."""
    out = skl.clone()
    out[:, bone_indices, 3] = out[:, bone_indices, 3] * factor
    return out


def edit_part_size(z, part_indices, factor):
    """demo.py:88: the norm of a part latent encodes the part's girth - scale it."""
    out = z.clone()
    out[:, part_indices, :] = out[:, part_indices, :] * factor
    return out


def edit_part_style(z, target_z, part_indices):
    """demo.py:90-95: keep each chosen part latent's norm, take its direction from `target_z`."""
    out = z.clone()
    for k in part_indices:
        norm = torch.sqrt(torch.sum(out[:, k, :] ** 2, dim=1, keepdim=True))
        tdir = target_z[:, k, :] / torch.sqrt(torch.sum(target_z[:, k, :] ** 2, dim=1, keepdim=True))
        out[:, k, :] = norm * tdir
    return out


def decode_edits(model, z, z_kps, tx, J_regressor, shape_idx, skl_idx, style_idx, bone_pairs, length_bones, parts,
                 length_factor=1.2, size_factor=1.2):
    """The edits of demo.py:64-103 for one (shape, skeleton-donor, style-donor) triple.
    z [n, 17, d], z_kps [n, 17, d] latents of the evaluated set, tx [n, N+1, 3] its meshes; `bone_pairs` are entries of
    NEWSKL_LIST whose orientation is transferred, `length_bones` indices whose length is scaled, `parts` part indices
    whose size / style is edited.  Returns a dict of decoded meshes [1, N+1, 3]."""
    dev = z.device
    J = torch.as_tensor(np.asarray(J_regressor, dtype=np.float32), device=dev)
    kps = torch.matmul(J, tx[:, :-1, :])
    skl = kps2skl(kps, "ori_m")
    sl = slice(shape_idx, shape_idx + 1)
    bone_idx = [constants.NEWSKL_LIST.index(list(b)) for b in bone_pairs]
    dummy = torch.zeros((1, 1, model.filters_enc[0][-1] if hasattr(model, "filters_enc") else 128), device=dev)
    with torch.no_grad():
        ori = skl2kps(edit_bone_orientation(skl[sl], skl[skl_idx:skl_idx + 1], bone_idx), "ori_m")
        length = skl2kps(edit_bone_length(skl[sl], length_bones, length_factor), "ori_m")
        out = {
            "rec_editpose": model.decode(z[sl], model.kps_encode(ori), dummy),
            "rec_editlength": model.decode(z[sl], model.kps_encode(length), dummy),
            "rec_editgirth": model.decode(edit_part_size(z[sl], parts, size_factor), z_kps[sl], dummy),
            "rec_editstyle": model.decode(edit_part_style(z[sl], z[style_idx:style_idx + 1], parts), z_kps[sl], dummy),
            "rec_shape": model.decode(z[sl], z_kps[sl], dummy),
            "rec_skl": model.decode(z[skl_idx:skl_idx + 1], z_kps[skl_idx:skl_idx + 1], dummy),
            "rec_style": model.decode(z[style_idx:style_idx + 1], z_kps[style_idx:style_idx + 1], dummy),
        }
    return out


def save_obj(obj_path, v, f, partcolor_list=None, vert_part_index=None):
    """utils_SH.py:163-195 without the skeleton overlay: 'v x y z r g b' lines (grey, or the part colour) + 1-based faces."""
    v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    f = f.detach().cpu().numpy() if torch.is_tensor(f) else np.asarray(f)
    with open(obj_path, "w") as fp:
        for i, p in enumerate(v):
            c = (192, 192, 192) if partcolor_list is None or vert_part_index is None else partcolor_list[int(vert_part_index[i])]
            fp.write("v %f %f %f %d %d %d\n" % (p[0], p[1], p[2], c[0], c[1], c[2]))
        for t in f + 1:
            fp.write("f %d %d %d\n" % (t[0], t[1], t[2]))


# ------------------------------------------------------------------------------------------------ fitting
def _face_table(faces, x_hat):
    """None, a scan.FaceTable or an integer array [nF, 3] -> None or a FaceTable for the decoded bodies x_hat (their last row is the
    dummy row), validated and uploaded here."""
    return faces if faces is None or isinstance(faces, scan.FaceTable) else scan.FaceTable(faces, x_hat.shape[1] - 1, x_hat.device)


def _default_dummy(model, z):
    """The decoder's dummy row as demo.py:74 makes it: zeros as wide as the decoder stack's input (its first conv's in_c)."""
    return torch.zeros((z.shape[0], 1, model.dconv[0].in_c), device=z.device)


def _decode(model, z, z_kps, dummy):
    if hasattr(model, "kps_encode"):                                   # SemanticHuman: decode(z, z_part_kps, dummy)
        return model.decode(z, z_kps, dummy)
    return model.decode(z)                                             # plain SpiralAutoencoder: decode(z)


def fit_latents(model, z, z_kps, objective, parts, *, steps, lr, dummy=None, after_step=None):
    """Optimise the latents `z[:, parts]` so that `objective(model.decode(...))` falls; returns (new z, loss per step).

    objective(x_hat) -> one scalar per body [B]; each step minimises their sum (bodies are independent).  Per step: decode ->
    objective -> backward to the moving latents -> the library's Adam (lr) on them; no host synchronisation.  Only z[:, parts]
    moves: the rest of z and z_kps are returned / left bitwise as given.  The model's parameters are frozen for the call (the
    decoder's backward pass computes no weight gradient) and their requires_grad flags restored afterwards; their .grad are not
    touched.  SemanticHuman: z [B, P, d], z_kps [B, P, d_kps], parts = part indices (None: all), dummy = the decoder's dummy row
    (None: zeros, as demo.py).  Plain SpiralAutoencoder: z [B, nz], z_kps ignored, parts = latent indices (None: all).
    The loss tensor [steps] stays on the device.  after_step(t), if given, is called after the optimiser step t (register_scan
    updates its pose there); it must not synchronise."""
    if steps < 1:
        raise ValueError("steps must be >= 1")
    semantic = hasattr(model, "kps_encode")
    z0 = z.detach()
    if not (z0.is_cuda and z0.dtype == torch.float32):
        raise RuntimeError("fit_latents: z must be an fp32 HIP tensor (got %s %s)" % (z0.device, z0.dtype))
    idx = torch.arange(z0.shape[1], device=z0.device) if parts is None else \
        torch.as_tensor(np.asarray(parts, dtype=np.int64).reshape(-1), device=z0.device)
    zk = z_kps.detach() if (semantic and z_kps is not None) else None
    if semantic and dummy is None:
        dummy = _default_dummy(model, z0)
    dummy = dummy.detach() if dummy is not None else None
    var = z0.index_select(1, idx).contiguous().requires_grad_(True)
    opt = optim.Adam([var], lr=lr)
    losses = torch.empty(steps, dtype=torch.float32, device=z0.device)
    params = list(model.parameters())
    flags = [p.requires_grad for p in params]
    try:
        for p in params:
            p.requires_grad_(False)
        for t in range(steps):
            x_hat = _decode(model, z0.index_copy(1, idx, var), zk, dummy)
            loss = objective(x_hat).sum()
            var.grad = None
            loss.backward()
            opt.step()
            losses[t] = loss.detach()
            if after_step is not None:
                after_step(t)
    finally:
        for p, f in zip(params, flags):
            p.requires_grad_(f)
    return z0.index_copy(1, idx, var.detach()), losses


def fit_part_girths(model, z, z_kps, rings, target, edit, hold=(), parts=None, bones=None, J=None, hold_lengths=False, *,
                    steps=200, lr=1e-2, dummy=None):
    """Edit bodies by their girths: ring `edit[i]` of body b should measure target[b, i]; the rings in `hold` keep the girth they
    have on decode(z); with hold_lengths, the lengths of `bones` (a measure.Bones or a bone list) on the joints J @ x_hat
    (measure.joints, J [K, N] on the device) keep theirs too.  The objective per body is the sum of squared relative errors.
    Batched: B bodies, each with its own targets, in one loop (fit_latents moves z[:, parts]).
    rings: a measure.GirthRings; target [B, len(edit)].  Returns (new z, girths [B, P] of the result, loss per step [steps])."""
    edit = [int(i) for i in np.asarray(edit).reshape(-1)]
    hold = [int(i) for i in np.asarray(hold, dtype=np.int64).reshape(-1)]
    dev = z.device
    target = torch.as_tensor(target, dtype=torch.float32, device=dev).reshape(z.shape[0], len(edit))
    if hold_lengths and (bones is None or J is None):
        raise ValueError("hold_lengths needs bones and J")
    if hold_lengths and not isinstance(bones, measure.Bones):
        bones = measure.Bones(bones, dev)
    if hold_lengths:
        J = torch.as_tensor(J, dtype=torch.float32, device=dev).contiguous()
    semantic = hasattr(model, "kps_encode")
    if semantic and dummy is None:
        dummy = _default_dummy(model, z)
    e_idx = torch.tensor(edit, dtype=torch.int64, device=dev)
    h_idx = torch.tensor(hold, dtype=torch.int64, device=dev)
    with torch.no_grad():
        x0 = _decode(model, z.detach(), z_kps, dummy)
        g_hold = measure.girths(x0, rings).index_select(1, h_idx)
        l_hold = measure.bone_lengths(measure.joints(x0, J), bones) if hold_lengths else None

    def objective(x_hat):
        g = measure.girths(x_hat, rings)
        err = ((g.index_select(1, e_idx) - target) / target).pow(2).sum(1)
        if hold:
            err = err + ((g.index_select(1, h_idx) - g_hold) / g_hold).pow(2).sum(1)
        if hold_lengths:
            ln = measure.bone_lengths(measure.joints(x_hat, J), bones)
            err = err + ((ln - l_hold) / l_hold).pow(2).sum(1)
        return err

    z_new, losses = fit_latents(model, z, z_kps, objective, parts, steps=steps, lr=lr, dummy=dummy)
    with torch.no_grad():
        g_final = measure.girths(_decode(model, z_new, z_kps, dummy), rings)
    return z_new, g_final, losses


def _visibility_cache(what, visibility, visibility_every):
    """The state scan._chamfer keeps between the passes of a fit: the last visibility mask and the pass counter."""
    every = int(visibility_every)
    if every < 1:
        raise ValueError("%s: visibility_every must be >= 1" % what)
    return None if visibility is None else {"every": every, "t": 0, "mask": None}


def _free_space_term(what, field, B, free_space_weight, silhouette_weight, margin, pose, vertex_mask=None):
    """The free-space arguments of a fit, checked -> None without a field, else x_hat -> free_space_weight * free +
    silhouette_weight * silhouette [B] (scan.free_space under `pose`, read afresh in every call, and the given vertex_mask).
    A rig field's way into its cameras (scan.free_space_cameras) is NOT read afresh: `term.pose_moved()` computes it - one launch -
    and the caller says so before the first step and after every change of `pose`; for a one-camera field it does nothing."""
    if field is None:
        return None
    scan._check_free_space_weights(what, field, B, margin, (("free_space_weight", free_space_weight), ("silhouette_weight", silhouette_weight)))
    if pose is not None and (not isinstance(pose, scan.Pose) or len(pose) != B):
        raise ValueError("%s: free_space_pose must be a scan.Pose of %d bodies" % (what, B))
    fw, sw, margin = float(free_space_weight), float(silhouette_weight), float(margin)
    rig = {}

    def term(x_hat):
        free, silhouette = scan.free_space(x_hat, field, pose=pose, vertex_mask=vertex_mask, margin=margin, **rig)
        return fw * free + sw * silhouette

    def pose_moved():
        if field.views is not None:
            rig["cameras"] = scan.free_space_cameras(field, pose)

    term.pose_moved = pose_moved
    return term


def fit_scan(model, z, z_kps, scans, parts=None, *, steps=200, lr=1e-2, trunc=None, w_model_to_scan=0.0, vertex_mask=None, dummy=None,
             faces=None, normal_angle=None, normal_faces=None, gate_on="vertices", visibility=None, visibility_faces=None,
             grazing_angle=None, visibility_every=1, robust=None, robust_scale=None, free_space=None, free_space_weight=1.0,
             silhouette_weight=1.0, free_space_margin=0.0, free_space_pose=None):
    """Fit bodies to unregistered point clouds: `fit_latents` with the objective scan.chamfer(decode(z), scans).  Each body has its
    own scan (a scan.ScanBatch, or a list of [m_b, 3] arrays / one [B, M, 3] array packed here once); no correspondence is needed.
    The scans must be in the model's normalised frame - nothing here aligns them; `register_scan` (or scan.align beforehand)
    solves for rotation, translation and scale.  trunc / w_model_to_scan / vertex_mask as in scan.chamfer (w_model_to_scan = 0: scan -> model only, for partial scans);
    the decoder's dummy row is never matched.  Works for both model classes (plain SpiralAutoencoder: z [B, nz], z_kps ignored);
    no host synchronisation in the loop.  faces: the model's triangles (a scan.FaceTable or an integer array [nF, 3]) - the scan
    -> model term is then the distance to the model's surface, not to its nearest vertex (scan.chamfer); a scan packed with
    order="morton" makes that search 2 - 3 times cheaper (DESIGN 4j has the measurement).  normal_angle / normal_faces: the normal
    gate of scan.chamfer (degrees; needs scans.normals, the model's triangles and trunc; None: none, the same bits as ever).
    gate_on: "vertices" (the default: that gate, on vertex normals, not built together with faces) or "surface" - the gate of the
    surface distance, on the face's normal (scan.chamfer; needs faces, normal_angle, scan normals and trunc).
    visibility: None (the default: everything above, bit for bit) or "viewpoint" - one-view scans: only the model vertices seen
    from scans.viewpoints take part (scan.chamfer(..., visibility=); visibility_faces / grazing_angle as there), which makes
    w_model_to_scan > 0 usable on them.  The mask is recomputed from the decoded body every `visibility_every`-th step (1: every
    step) and reused in between; the returned Chamfer value uses a fresh one.  A pass costs about half a vertex fit step at B = 64
    (DESIGN 4q): 1 while pose or shape still move, 4 once the fit has settled.
    robust / robust_scale: None (the default - off: everything above, bit for bit) or the robust data term of scan.chamfer
    ("geman-mcclure" / "huber" with sigma in the model's normalised units): scan points far from the body - clothing, hair, a
    floor patch - fade out of value and gradient instead of dominating them.
    free_space: None (the default - off: everything above, bit for bit, the same launches) or a scan.DepthField of the depth
    images the scans came from.  The objective gains free_space_weight * free + silhouette_weight * silhouette of
    scan.free_space(decode(z), free_space, pose=free_space_pose, margin=free_space_margin): model vertices in space the sensor
    saw through, or projecting outside the body's silhouette, are pushed back - the data term a one-view fit lacks for the half
    of the body that visibility= only removes (two launches per step).  free_space_pose: the scan.Pose (camera frame
    -> model frame) that brought the scans into the model's frame, None when the model's frame is the camera's.  A given
    vertex_mask holds for the term too; the mask of visibility= does not - the unseen vertices are the ones it is for.  Nearest-pixel sampling, no image gradient, no robust form; a field made with distortion= is read through its lens model (scan.free_space).  The loss per step
    includes the term; the returned Chamfer value does not.  ValueError for a field of another batch size, a negative weight or
    margin.  A rig field (scan.DepthField.from_depth(..., extrinsics=)) charges every vertex under each of the rig's cameras:
    free_space_pose is then rig frame -> model frame, the way into the cameras is computed once before the loop
    (scan.free_space_cameras), and a step adds one forward and one backward launch for all cameras.
    Returns (new z, chamfer [B] of the result, loss per step [steps])."""
    if not isinstance(scans, scan.ScanBatch):
        scans = scan.ScanBatch(scans, z.device)
    if len(scans) != z.shape[0]:
        raise ValueError("fit_scan: %d bodies, %d scans" % (z.shape[0], len(scans)))
    scan._MatchPlan.check_gate("fit_scan", gate_on, normal_angle, faces, scans, trunc)
    scan._MatchPlan.check_visibility("fit_scan", visibility, visibility_faces, faces, normal_faces, grazing_angle, scans)
    vis_cache = _visibility_cache("fit_scan", visibility, visibility_every)
    rb = {} if scan._robust_arg("fit_scan", robust, robust_scale) is None else dict(robust=robust, robust_scale=robust_scale)
    extra = _free_space_term("fit_scan", free_space, z.shape[0], free_space_weight, silhouette_weight, free_space_margin, free_space_pose, vertex_mask)
    semantic = hasattr(model, "kps_encode")
    if semantic and dummy is None:
        dummy = _default_dummy(model, z)
    tables = {}

    def data(x_hat):
        if not tables:                                                     # validated and uploaded once, at the first decode: n is known here
            tables.update(faces=_face_table(faces, x_hat), normal_faces=_face_table(normal_faces, x_hat) if normal_angle is not None else None)
            if visibility is not None:
                vf = visibility_faces if visibility_faces is not None else (faces if faces is not None else normal_faces)
                tables.update(visibility_faces=tables["faces"] if vf is faces else _face_table(vf, x_hat))
        if visibility is None:
            return scan.chamfer(x_hat, scans, None, vertex_mask, trunc, w_model_to_scan, normal_angle=normal_angle, gate_on=gate_on, **tables, **rb)
        return scan._chamfer(x_hat, scans, None, vertex_mask, trunc, w_model_to_scan, None, tables["faces"], normal_angle, tables["normal_faces"],
                             gate_on, visibility=visibility, visibility_faces=tables["visibility_faces"], grazing_angle=grazing_angle,
                             vis_cache=vis_cache, **rb)

    objective = data if extra is None else (lambda x_hat: data(x_hat) + extra(x_hat))
    if extra is not None:
        extra.pose_moved()                                                 # a rig field: its cameras once, the pose is fixed
    z_new, losses = fit_latents(model, z, z_kps, objective, parts, steps=steps, lr=lr, dummy=dummy)
    with torch.no_grad():
        if vis_cache is not None:
            vis_cache["t"] = 0                                             # the result is measured under a fresh mask
        final = data(_decode(model, z_new, z_kps, dummy))                  # the Chamfer value alone
    return z_new, final, losses


def register_scan(model, z, z_kps, scans, parts=None, *, mode="similarity", init="moments", align_iters=30, align_every=1, steps=200,
                  lr=1e-2, trunc=None, w_model_to_scan=0.0, align_w_model_to_scan=None, vertex_mask=None, dummy=None, faces=None,
                  normal_angle=None, normal_faces=None, align_on="vertices", align_step="point", gate_on="vertices", visibility=None,
                  visibility_faces=None, grazing_angle=None, visibility_every=1, robust=None, robust_scale=None, free_space=None,
                  free_space_weight=1.0, silhouette_weight=1.0, free_space_margin=0.0):
    """`fit_scan` for scans in their own frame and units: solves for the pose (scan frame -> model frame, a scan.Pose) together
    with the latents.

    1. scan.align of the scans against decode(z): `align_iters` ICP iterations in `mode` from the start `init`, with
       align_w_model_to_scan (None: 1.0 for mode "similarity", else the fit's own w_model_to_scan).  align_iters = 0 keeps the
       start pose as it is.
    2. The fit_latents loop with the Chamfer objective on the aligned scans (trunc / w_model_to_scan / vertex_mask as in
       fit_scan).  After every `align_every`-th step the pose is updated from the matches that step's forward pass has just found
       (moments -> closed-form increment -> the ORIGINAL scan under the new pose: three launches, no search); align_every = 0
       keeps the pose of stage 1.  No host synchronisation in the loop.

    Returns (new z, pose, chamfer [B] of the result in the model's frame, loss per step [steps]).  `pose.apply(scans)` are the
    scans in the model's frame, `pose.to_scan_frame(decode(z_new))` the fitted body in the scan's.

    Limits: those of scan.align - ICP is local (the moment start fixes translation and scale, not rotation; beyond about 45
    degrees pass a start Pose), a similarity with w_model_to_scan = 0 from the identity can shrink the scan into the model (the
    defaults of stage 1 avoid it), partial scans want mode="rigid" with scan -> model only, and only the normalisations that are
    similarities (zeromean, zeroroot, onelength, small) can be undone by a pose.  faces (as in fit_scan) makes the FIT's scan ->
    model term point-to-surface.  align_on: "vertices" (the default) - both pose stages work on vertex pairs, whatever the fit
    measures; "surface" (needs faces) - both work on (scan point, foot point on the surface) pairs: stage 1 is
    scan.align(..., faces=) and the in-loop update is scan.pose_update(..., surface=True) on the foot points the step's forward
    pass has just found, so fit and pose lower one and the same surface Chamfer value.  normal_angle /
    normal_faces: the normal gate of scan.chamfer on every search of both stages (needs scans.normals, the model's triangles and
    trunc; the scan's normals follow the pose's rotation; None: none, the same bits as ever).  align_step: "point" (the default:
    everything above, bit for bit) or "plane" - both pose stages take the linearised point-to-plane step (scan.align(...,
    step="plane") and scan.pose_update(..., step="plane")) on the pairs `align_on` selects; it needs the model's triangles for the
    normals (faces, or normal_faces).  That step is Gauss-Newton, so a pose update is not guaranteed to lower the Chamfer value, and
    a body whose system is singular (too few or parallel normals) keeps its pose for that update.  gate_on: "vertices" (the
    default: the gate above, on vertex normals, not built together with faces) or "surface" - the fit's surface distance is gated
    by the face's normal (scan.chamfer(..., gate_on="surface"); needs faces, normal_angle, scan normals and trunc), with either
    align_on: "surface" gates both pose stages' foot points the same way, "vertices" runs them on vertex pairs gated by the
    vertex normals (of normal_faces, or of faces when that is omitted).  visibility: None (the default: everything above, bit
    for bit) or "viewpoint" - one-view scans: scans.viewpoints, in the SCAN's frame, follow the pose; stage 1 is
    scan.align(..., visibility=) (a fresh mask every iteration), the fit uses scan.chamfer(..., visibility=) on the aligned
    batch with the mask recomputed every `visibility_every`-th step, and every in-loop pose update moves the viewpoint with the
    scan.  visibility_faces / grazing_angle as in scan.chamfer.  robust / robust_scale: None (the default - off: everything
    above, bit for bit) or the robust term of scan.chamfer, in all three places: stage 1 is scan.align(..., robust=) (IRLS), the
    fit's objective is the robust Chamfer value, and every in-loop pose update weighs its pairs the same way.  free_space /
    free_space_weight / silhouette_weight / free_space_margin: None (the default - off: everything above, bit for bit, the same
    launches) or the free-space and silhouette terms of fit_scan, for scans that are depth images in the camera's frame (the
    scan's frame): the term of every step is scan.free_space(decode(z), free_space, pose=the pose as it stands), so it follows
    every in-loop pose update.  The term moves the latents only - it does NOT move the pose: stage 1 (scan.align) and the in-loop
    pose updates are what they are without it.  The loss per step includes the term; the returned Chamfer value does not.
    ValueError for a field of another batch size, a negative weight or margin.  A rig field (scans in the rig's frame) works the
    same way; its cameras are recomputed - one launch - after stage 1 and after every in-loop pose update.  No file
    reader."""
    if not isinstance(scans, scan.ScanBatch):
        scans = scan.ScanBatch(scans, z.device)
    if len(scans) != z.shape[0]:
        raise ValueError("register_scan: %d bodies, %d scans" % (z.shape[0], len(scans)))
    if mode not in ("translation", "rigid", "similarity"):
        raise ValueError("register_scan: mode must be 'translation', 'rigid' or 'similarity'")
    align_iters, align_every = int(align_iters), int(align_every)
    if align_iters < 0 or align_every < 0:
        raise ValueError("register_scan: align_iters and align_every must be >= 0")
    if align_on not in ("vertices", "surface"):
        raise ValueError("register_scan: align_on must be 'vertices' or 'surface'")
    if align_step not in ("point", "plane"):
        raise ValueError("register_scan: align_step must be 'point' or 'plane'")
    if align_step == "plane" and faces is None and normal_faces is None:
        raise ValueError("register_scan: align_step='plane' needs the model's triangles (faces or normal_faces)")
    on_surface = align_on == "surface"
    if on_surface and faces is None:
        raise ValueError("register_scan: align_on='surface' needs faces (the model's triangles)")
    surface_gate = scan._MatchPlan.check_gate("register_scan", gate_on, normal_angle, faces, scans, trunc) is not None
    scan._MatchPlan.check_visibility("register_scan", visibility, visibility_faces, faces, normal_faces, grazing_angle, scans)
    vis_cache = _visibility_cache("register_scan", visibility, visibility_every)
    rb = {} if scan._robust_arg("register_scan", robust, robust_scale) is None else dict(robust=robust, robust_scale=robust_scale)
    if free_space is not None:                                                          # checked before the device is used; the pose comes below
        _free_space_term("register_scan", free_space, z.shape[0], free_space_weight, silhouette_weight, free_space_margin, None)
    semantic = hasattr(model, "kps_encode")
    if semantic and dummy is None:
        dummy = _default_dummy(model, z)
    w_align = (1.0 if mode == "similarity" else w_model_to_scan) if align_w_model_to_scan is None else align_w_model_to_scan
    with torch.no_grad():
        x0 = _decode(model, z.detach(), z_kps, dummy)
    if normal_angle is not None and faces is not None and not surface_gate:              # stage 1 on vertex pairs would run before scan.chamfer says so
        raise ValueError("register_scan: normal_angle together with faces= (the surface distance) is not built for the gate on vertex "
                         "normals; gate_on='surface' gates the surface search by the face's normal")
    normal_faces, faces = _face_table(normal_faces, x0), _face_table(faces, x0)
    if visibility is not None:
        vf = visibility_faces if visibility_faces is not None else (faces if faces is not None else normal_faces)
        visibility_faces = faces if vf is faces else _face_table(vf, x0)
    if normal_faces is None:                                                            # the vertex normals' table falls back to the surface's
        normal_faces = faces
    vis = {} if visibility is None else dict(visibility=visibility, visibility_faces=visibility_faces, grazing_angle=grazing_angle)
    pose, aligned, _ = scan.align(x0, scans, mode=mode, iters=align_iters, init=init, trunc=trunc, w_model_to_scan=w_align,
                                  vertex_mask=vertex_mask, normal_angle=normal_angle, normal_faces=normal_faces,
                                  faces=faces if on_surface else None, step=align_step, gate_on=gate_on if on_surface else "vertices", **vis, **rb)
    matches = {} if align_every > 0 else None
    state = {"partials": None}

    extra = _free_space_term("register_scan", free_space, z.shape[0], free_space_weight, silhouette_weight, free_space_margin, pose, vertex_mask)

    def data(x_hat):                                                                    # foot-point pose updates read no vertex record
        if visibility is not None:
            return scan._chamfer(x_hat, aligned, None, vertex_mask, trunc, w_model_to_scan, matches, faces, normal_angle, normal_faces, gate_on,
                                 vertex_matches=not on_surface, vis_cache=vis_cache, **vis, **rb)
        return scan._chamfer(x_hat, aligned, None, vertex_mask, trunc, w_model_to_scan, matches, faces, normal_angle, normal_faces, gate_on,
                             vertex_matches=not on_surface, **rb)

    objective = data if extra is None else (lambda x_hat: data(x_hat) + extra(x_hat))  # `pose` is updated in place: the term reads it afresh
    if extra is not None:
        extra.pose_moved()                                                              # a rig field's cameras under the pose of stage 1

    def after_step(t):
        if (t + 1) % align_every == 0:
            state["partials"] = scan.pose_update(pose, scans, aligned, matches, mode, partials=state["partials"], surface=on_surface,
                                                 step=align_step, **rb)
            if extra is not None:
                extra.pose_moved()                                                      # ... and under every pose after it: one launch

    z_new, losses = fit_latents(model, z, z_kps, objective, parts, steps=steps, lr=lr, dummy=dummy,
                                after_step=after_step if align_every > 0 else None)
    with torch.no_grad():
        final = scan.chamfer(_decode(model, z_new, z_kps, dummy), aligned, None, vertex_mask, trunc, w_model_to_scan, faces=faces,
                             normal_angle=normal_angle, normal_faces=normal_faces, gate_on=gate_on, **vis, **rb)
    return z_new, pose, final, losses
