"""The three-plane kernels (csrc/p3_conv.hip, csrc/wgrad_p3.hip) against float64 over the shapes their predicates accept, not only
the shipped model's: batches 16 ... 1024, spirals of 1 ... 64 entries, gathered channels 16 ... 256, output channels that are any
multiple of 4 (partial 16-channel tiles), the weight-streaming form with and without K padding, the two-row-tile forms, ragged and
grouped lists, and the weight gradient's channel-tile and column-group widths.

Every accepted point of GRID runs each entry point that takes it three ways - the exact fp32 kernel, the plane kernel and a float64
gather-matmul on the device - under the gate of tests/test_p3.py,

    max|y_p3 - y_f64|  <=  1.5 max|y_exact - y_f64| + 2^-23 max|y_f64|,    max|y_exact - y_f64| <= 1e-5 (1e-4 gradients) max|y_f64|,

on training-scale and adversarial operands (six decades of magnitude, sums that cancel in every entry point).  The gate holds each
form's sum (identity activation) and weight gradient; the fused epilogues (bias, the six activations, the dummy row, the activation
derivative from yprev or from its image) are then held, element by element, to that form's own error on the sum times the
activation's slope, plus the fp32 evaluation of the activation (_Rec.gate_act).  Images the kernels write are the images of what they store, bit for bit; rows a kernel
must not read hold NaN.  Every rejected point is refused by every entry point without a launch, and the profiler names seen over
the sweep cover every template instantiation the dispatch can reach."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib
from semantichuman_amd.stack import ConvStep

from tests.p3_ref import (ACT64, DACT64, SH_ERR_UNSUPPORTED, act_slope64, arr, decode_image, has_image, local_table, rnd, to_p3,
                          wfrag3)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
RT2_TILES = 16384           # R * B / 16 from which the resident kernels take two-row tiles on a 256-CU MI355X (choose_p3)

# (name, B, R, n_in, S, Cg, Nout, tags).  Forward: a layer Cin = Cg -> Cout = Nout gathering n_in rows into R; backward-data: the
# layer Cin = Nout -> Cout = Cg over the same table (dpre has R rows, dx n_in); weight gradient: view "wA" = the forward layer,
# "wB" = the backward one.  Tags = what the library's predicates make of the point (test_grid_points_reach_their_kernels), except
# rt2f / rt2b, which restate the dispatch's rule at the MI355X's 256 CUs (its CU count is read on the device, so only the GPU
# coverage test, test_sweep_covers_every_reachable_instantiation, sees the library take two-row tiles):
#   res / str / rej    resident weight (conv_p3_kernel), streamed weight (conv_p3s_kernel), refused
#   rt2f / rt2b        forward / backward-data at R * B / 16 >= RT2_TILES on a resident weight (two-row tiles)
#   rag                backward-data over ragged lists (conv_p3r_kernel)
#   fg2 / fg4, bg2 / bg4   grouped lists of 2 or 4 members, forward / backward (conv_p3g_kernel; 16 gathered channels included)
#   wA / wB            weight gradient in the plane form (wgrad_p3_kernel)
GRID = [
    # 16 gathered channels, resident: one or two channel tiles, spirals 1 ... 64, partial output tiles
    ("c16_s1_n4", 16, 97, 131, 1, 16, 4, "res fg4 bg4"),
    ("c16_s3_n12", 48, 120, 100, 3, 16, 12, "res fg4 bg4"),
    ("c16_s8_n20", 80, 64, 90, 8, 16, 20, "res fg4 bg4"),
    ("c16_s9_n32", 64, 77, 77, 9, 16, 32, "res fg4 bg4 wA"),
    ("c16_s12_n16", 272, 41, 60, 12, 16, 16, "res fg4 bg4"),
    ("c16_s18_n32", 16, 150, 150, 18, 16, 32, "res fg4 bg4 wA"),
    ("c16_s25_n4", 48, 70, 90, 25, 16, 4, "res fg4 bg4"),
    ("c16_s33_n16", 16, 60, 60, 33, 16, 16, "res fg4 bg4"),
    ("c16_s64_n12", 32, 50, 80, 64, 16, 12, "res fg4 bg4"),
    # wider gathers, resident: 1, 2, 4 and 8 channel tiles
    ("s8_c32_n36", 64, 130, 200, 8, 32, 36, "res rag fg2 bg2"),
    ("s9_c32_n48", 16, 90, 90, 9, 32, 48, "res rag fg2 bg2"),
    ("s3_c32_n128", 80, 100, 140, 3, 32, 128, "res wA wB"),
    ("s6_c32_n96", 64, 100, 100, 6, 32, 96, "res wA wB"),
    ("s4_c96_n64", 64, 100, 120, 4, 96, 64, "res rag fg2 bg2 wA wB"),
    ("s1_c256_n64", 48, 80, 80, 1, 256, 64, "res rag fg2 bg2 wA wB"),
    ("s12_c32_n12", 16, 110, 110, 12, 32, 12, "res rag fg4 bg4"),
    ("s5_c160_n20", 32, 90, 100, 5, 160, 20, "res rag fg4 bg4"),
    ("s25_c64_n16", 48, 80, 120, 25, 64, 16, "res rag fg4 bg4 wB"),
    ("s3_c128_n32", 64, 120, 120, 3, 128, 32, "res rag fg4 bg4 wA wB"),
    # streamed weight: K padded to whole chunks or not, 32 output channels (two tiles), several output slices
    ("str_s12_c64_n64", 64, 150, 150, 12, 64, 64, "str wA wB"),
    ("str_s25_c32_n64", 48, 110, 140, 25, 32, 64, "str wA wB"),
    ("str_s9_c256_n32", 16, 71, 90, 9, 256, 32, "str wA wB"),
    ("str_s25_c64_n32", 32, 60, 80, 25, 64, 32, "str wA wB"),
    ("str_s7_c96_n64", 32, 80, 100, 7, 96, 64, "str wA wB"),
    ("str_s5_c160_n192", 80, 60, 70, 5, 160, 192, "str wA wB"),
    ("str_s12_c128_n128", 16, 91, 90, 12, 128, 128, "str wA wB"),
    # two-row tiles (R * B / 16 >= 16 384): odd R leaves the last tile half empty
    ("rt2_c16_n16", 1024, 257, 300, 3, 16, 16, "res rt2f rt2b fg4 bg4"),
    ("rt2_c16_n32", 1024, 257, 300, 9, 16, 32, "res rt2f rt2b fg4 bg4 wA"),
    ("rt2_c32_n16", 1024, 257, 300, 4, 32, 16, "res rt2f rt2b rag fg4 bg4 wB"),
    ("rt2_c64_n20", 1024, 257, 300, 5, 64, 20, "res rt2f rt2b rag fg4 bg4"),
    ("rt2_c32_n52", 1024, 257, 300, 6, 32, 52, "res rt2f rt2b rag fg2 bg2"),
    ("rt2_b272_c96_n36", 272, 964, 964, 3, 96, 36, "res rt2f rt2b rag fg2 bg2"),
    # weight gradients with R smaller than one tile; odd unit counts R * B / 16 (3, 15, 71, 91) complete with the zero row
    ("w_r1", 32, 1, 7, 3, 32, 32, "res rag fg4 bg4 wA wB"),
    ("w_r2", 16, 2, 9, 5, 32, 64, "res rag fg2 bg2 wA wB"),
    ("w_r3", 16, 3, 11, 4, 64, 32, "res rag fg4 bg4 wA wB"),
    ("w_r4", 80, 4, 12, 9, 16, 32, "res fg4 bg4 wA"),
    ("w_r5", 48, 5, 16, 3, 96, 96, "rej wA wB"),
    # refused: batch, output channels, gathered channels, spiral length, unbuilt 16-channel tiles, no resident or streaming form
    ("rej_b40", 40, 60, 60, 8, 32, 32, "rej"),
    ("rej_n30", 64, 60, 60, 8, 32, 30, "rej"),
    ("rej_c48", 64, 60, 60, 8, 48, 32, "rej"),
    ("rej_s65", 64, 60, 60, 65, 16, 16, "rej"),
    ("rej_c16_n64", 64, 70, 90, 9, 16, 64, "rej wA"),
    ("rej_c96_n96", 48, 60, 80, 9, 96, 96, "rej wA wB"),
]
NAMES = [g[0] for g in GRID]


def _steps(g, device=None):
    """The library's own tables for the point: the forward layer (Cg -> Nout) and the backward one (Nout -> Cg)."""
    name, B, R, n_in, S, Cg, Nout, _ = g
    table = local_table(np.random.default_rng(zlib.crc32(name.encode())), R, n_in, S)
    fs = ConvStep(param=0, table=table, n_in=n_in, cin=Cg, cout=Nout, act=2, dead_dummy_grad=True).finalize()
    bs = ConvStep(param=0, table=table, n_in=n_in, cin=Nout, cout=Cg, act=2, dead_dummy_grad=True).finalize()
    if device is not None:
        fs.to(device)
        bs.to(device)
    return fs, bs


def _tags(g, fs, bs):
    """What the library's predicates make of a point (the GRID tags' vocabulary)."""
    lib = _lib.load()
    name, B, R, n_in, S, Cg, Nout, _ = g
    t = set()
    kind = lib.sh_spiral_conv_p3_kind(B, S, Cg, Nout)
    t.add({0: "rej", 1: "res", 2: "str"}[kind])
    if kind == 1 and R * (B // 16) >= RT2_TILES:
        t.add("rt2f")
    if kind == 1 and n_in * (B // 16) >= RT2_TILES:
        t.add("rt2b")
    if bs.rag is not None and lib.sh_spiral_conv_p3_rag_ok(B, S, Cg, Nout, int(bs.rag[0].shape[1])):
        t.add("rag")
    if fs.fgrp is not None and lib.sh_spiral_conv_p3_grp_ok(B, S, Cg, Nout, int(fs.fgrp[0].shape[1])):
        t.add("fg%d" % lib.sh_spiral_conv_p3_grp_members(B, S, Cg, Nout))
    if bs.bgrp is not None and lib.sh_spiral_conv_p3_grp_ok(B, S, Cg, Nout, int(bs.bgrp[0].shape[1])):
        t.add("bg%d" % lib.sh_spiral_conv_p3_grp_members(B, S, Cg, Nout))
    if lib.sh_spiral_conv_bwd_wgt_p3_ok(B, R, S, Cg, Nout):
        t.add("wA")
    if lib.sh_spiral_conv_bwd_wgt_p3_ok(B, R, S, Nout, Cg):
        t.add("wB")
    return t


def test_grid_points_reach_their_kernels():
    """CPU: the library's predicates classify every grid point as the grid says, so a predicate change that moves a point out of the
    kernel it is there for fails here instead of quietly dropping coverage."""
    bad = []
    for g in GRID:
        fs, bs = _steps(g)
        got, want = _tags(g, fs, bs), set(g[7].split())
        if got != want:
            bad.append((g[0], sorted(got), sorted(want)))
    assert not bad, bad
    tags = [set(g[7].split()) for g in GRID]
    # the grid's reach (the issue's table): batches, spirals, channels, forms
    acc = [g for g, t in zip(GRID, tags) if "rej" not in t]
    assert {16, 48, 80, 272, 1024} <= {g[1] for g in acc}
    assert {1, 3, 8, 9, 12, 18, 25, 33, 64} <= {g[4] for g in acc if g[5] == 16}
    assert {16, 32, 64, 96, 128, 160, 256} <= {g[5] for g in acc}
    assert {4, 12, 16, 20, 32, 36, 48, 64, 96, 128, 192} <= {g[6] for g in acc}
    assert {1, 2, 3, 4, 5} <= {g[2] for g, t in zip(GRID, tags) if "wA" in t or "wB" in t}
    assert any(g[1] * g[2] // 16 % 2 for g, t in zip(GRID, tags) if "wA" in t or "wB" in t)


# ------------------------------------------------------------------------------------------------------------------- the sweep
FAMILY_NAMES = ["fwd conv_p3", "fwd conv_p3s", "fwd conv_p3g", "bwd conv_p3", "bwd conv_p3 f32r", "bwd conv_p3s", "bwd conv_p3r",
                "bwd conv_p3g", "wgrad_p3 dW", "wgrad_p3 dbias"]


class _Rec:
    def __init__(self):
        self.fail = []          # (what, detail)
        self.ratio = {}         # family -> worst err_p3 / err_exact
        self.n = {}             # family -> checks

    def gate(self, what, fam, got, exact, ref, tol_exact):
        """The gate of tests/test_p3.py on a sum (identity activation) or a weight gradient; returns the planes' error."""
        scale = float(ref.abs().max())
        if not (bool(torch.isfinite(got).all()) and bool(torch.isfinite(exact).all())):
            self.fail.append((what, "non-finite values"))
            return float("inf")
        e3 = float((got.double() - ref).abs().max())
        ex = float((exact.double() - ref).abs().max())
        if not e3 <= 1.5 * ex + 2.0 ** -23 * scale:
            self.fail.append((what, "planes %.3e > 1.5 x exact %.3e + 2^-23 x %.3e" % (e3, ex, scale)))
        if not ex <= tol_exact * scale:
            self.fail.append((what, "exact %.3e > %.0e x %.3e" % (ex, tol_exact, scale)))
        r = e3 / ex if ex > 0 else (0.0 if e3 == 0 else float("inf"))
        self.ratio[fam] = max(self.ratio.get(fam, 0.0), r)
        self.n[fam] = self.n.get(fam, 0) + 1
        return e3

    def gate_act(self, what, got, ref, slope, e_sum):
        """An activated result (or a gradient times the activation derivative) of a form whose sum - the same accumulator, bit for
        bit: the kernels are deterministic - was e_sum away from float64 in its identity run, which passed the gate above.  Element by
        element the result may then be off by slope x e_sum (slope: the activation's largest slope within e_sum of the float64 sum,
        or the derivative factor) plus the fp32 evaluation of the activation itself (a few roundings of the element, one ulp of the
        result's scale).  A saturated sigmoid is held to its ulps; a wrong activation, channel or row fails."""
        if not bool(torch.isfinite(got).all()):
            self.fail.append((what, "non-finite values"))
            return
        err = (got.double() - ref).abs()
        allow = slope * e_sum + 2.0 ** -21 * ref.abs() + 2.0 ** -23 * float(ref.abs().max())
        if bool((err > allow).any()):
            i = int(torch.argmax(err - allow))
            self.fail.append((what, "error %.3e > allowed %.3e at element %d (e_sum %.3e)" % (float(err.flatten()[i]), float(allow.flatten()[i]),
                                                                                           i, e_sum)))

    def same(self, what, a, b):
        if not torch.equal(a, b):
            self.fail.append((what, "not bitwise equal"))

    def zero_row(self, what, y, row):
        if row >= 0 and not bool((y[row] == 0).all()):
            self.fail.append((what, "dummy row %d is not exactly 0" % row))


def _check(rc, what):
    _lib.check(rc, what)


def _fwd(rec, g, fs, w, bias, x, wf):
    lib, d = _lib.load(), x.device
    name, B, R, n_in, S, Cg, Nout, _ = g
    table = fs.dev["table"]
    fam = "fwd conv_p3s" if lib.sh_spiral_conv_p3_kind(B, S, Cg, Nout) == 2 else "fwd conv_p3"
    x64, w64 = x.double(), w.double().view(Nout, S, Cg)
    pre = torch.zeros((R, B, Nout), dtype=torch.float64, device=d)
    tl = table.long()
    for s in range(S):
        pre += x64[tl[:, s]] @ w64[:, s, :].t()
    pre += bias.double()
    del x64
    xp = to_p3(x)
    img = has_image(Nout)
    grp = fs.dev.get("fgrp")
    use_grp = grp is not None and lib.sh_spiral_conv_p3_grp_ok(B, S, Cg, Nout, int(grp[0].shape[1]))
    from semantichuman_amd import ops
    e0 = {}
    for act in range(6):
        zr = R - 1
        ref = ACT64[act](pre)
        ref[zr] = 0
        ye = torch.full((R, B, Nout), NAN, device=d)
        _lib.set_f32_mma_mode("exact")
        ops.spiral_conv_fwd(x, "vm", table, w, bias, ye, "vm", R, S, act, zr)
        tag = "%s fwd act %d" % (name, act)
        y = torch.full((R, B, Nout), NAN, device=d)
        yp = torch.full((lib.sh_p3_bytes(R, B, Nout),), 255, dtype=torch.uint8, device=d) if img else None
        _check(lib.sh_spiral_conv_fwd_p3(_lib.ptr(xp), _lib.ptr(table), _lib.ptr(wf), _lib.ptr(bias), _lib.ptr(y), B * Nout, Nout, _lib.ptr(yp),
                                         B, R, S, Cg, Nout, act, zr, _lib.stream_ptr()), tag)
        outs = {"exact": ye, "planes": y}
        if use_grp:
            g_r, g_p, g_o = grp
            yg = torch.full((R, B, Nout), NAN, device=d)
            ypg = torch.full_like(yp, 255) if img else None
            _check(lib.sh_spiral_conv_p3_grp(_lib.ptr(xp), _lib.ptr(g_r), _lib.ptr(g_p), _lib.ptr(g_o), int(g_r.shape[0]), int(g_r.shape[1]),
                                             _lib.ptr(wf), _lib.ptr(bias), _lib.ptr(yg), B * Nout, Nout, _lib.ptr(ypg), None, 0, 0, None, act, zr, 0,
                                             B, R, S, Cg, Nout, _lib.stream_ptr()), tag + " grouped")
            outs["grouped"] = yg
            if img:
                rec.same(tag + " grouped image", ypg, to_p3(yg))
        if img:
            rec.same(tag + " image", yp, to_p3(y))
        if act == 0:
            e0["exact"] = float((ye.double() - ref).abs().max())
            e0["planes"] = rec.gate(tag, fam, y, ye, ref, 1e-5)
            if use_grp:
                e0["grouped"] = rec.gate(tag + " grouped", "fwd conv_p3g", yg, ye, ref, 1e-5)
        for k, v in outs.items():
            if act:
                rec.gate_act("%s %s" % (tag, k), v, ref, act_slope64(act, pre, e0[k]), e0[k])
            rec.zero_row("%s %s" % (tag, k), v, zr)


def _bwd(rec, g, bs, w, dp, yprev_src, wf):
    """Backward-data of the layer Nout -> Cg (w [Cg][S*Nout]); dp [R + n_extra][B][Cg] with the dummy row R - 1 zero and the
    pre-summed rows filled by the caller."""
    lib, d = _lib.load(), dp.device
    name, B, R, n_in, S, Cg, Nout, _ = g
    from semantichuman_amd import ops
    table, table_t = bs.dev["table"], bs.dev["table_t"]
    kind = lib.sh_spiral_conv_p3_kind(B, S, Cg, Nout)
    n_ext = dp.shape[0]
    # float64: the scatter form over the FORWARD table (no transposed table, no pre-sums); the dummy input row's gradient is dropped
    w64 = w.double().view(Cg, S, Nout)
    pre = torch.zeros((n_in, B, Nout), dtype=torch.float64, device=d)
    dp64 = dp[:R].double()
    tl = table.long()
    for s in range(S):
        pre.index_add_(0, tl[:, s], dp64 @ w64[:, s, :])
    pre[n_in - 1] = 0
    del dp64
    img_full = to_p3(dp)                                             # every row imaged
    # rows >= R without an image: image rows behind R and fp32 rows below R hold NaN
    img_part = to_p3(dp[:R].contiguous(), rows=n_ext)
    img_part[lib.sh_p3_bytes(R, B, Cg):] = 255
    f32_part = dp.clone()
    f32_part[:R] = NAN
    wt = ops.weight_transpose(w, S, Nout, Cg)
    img_out = has_image(Nout)
    rag = bs.rag is not None and lib.sh_spiral_conv_p3_rag_ok(B, S, Cg, Nout, int(bs.rag[0].shape[1]))
    grp = bs.dev.get("bgrp")
    # grouped lists need no one-row list kernel (16 gathered channels: sh_stack_plan_f32 takes the grouped form where the ragged one is refused)
    use_grp = grp is not None and lib.sh_spiral_conv_p3_grp_ok(B, S, Cg, Nout, int(grp[0].shape[1]))
    nb_out = lib.sh_p3_bytes(n_in, B, Nout) if img_out else 0
    e0 = {}
    for act in range(6):
        yprev = None if act == 0 else yprev_src[act]
        zr = -1 if act == 0 else n_in - 1
        ref = pre if act == 0 else pre * DACT64[act](yprev.double())
        if zr >= 0:
            ref = ref.clone()
            ref[zr] = 0
        tag = "%s bwd act %d" % (name, act)
        _lib.set_f32_mma_mode("exact")
        de = torch.full((n_in, B, Nout), NAN, device=d)
        ops.spiral_conv_bwd_data(dp, "vm", table_t, wt, de, "vm", yprev, "vm", act, zr, n_in, S, Nout, Cg)
        slope = None if act == 0 else DACT64[act](yprev.double()).abs()

        def check(key, fam, got):
            """identity: the gate (and this form's error on the sum); a derivative factor: that error times the factor"""
            if act == 0:
                e0[key] = rec.gate("%s %s" % (tag, key), fam, got, de, ref, 1e-4)
            else:
                rec.gate_act("%s %s" % (tag, key), got, ref, slope, e0[key])
            rec.zero_row("%s %s" % (tag, key), got, zr)

        if act == 0:
            e0["exact"] = float((de.double() - ref).abs().max())
        else:
            rec.gate_act(tag + " exact", de, ref, slope, e0["exact"])
        ysv = B * Nout if yprev is not None else 0
        ysb = Nout if yprev is not None else 0
        yimg = to_p3(yprev) if (yprev is not None and img_out) else None

        def dense(xp, xf, n_img, yp_planes, what):
            dx = torch.full((n_in, B, Nout), NAN, device=d)
            dxp = torch.full((nb_out,), 255, dtype=torch.uint8, device=d) if img_out else None
            _check(lib.sh_spiral_conv_bwd_data_p3(_lib.ptr(xp), R - 1, _lib.ptr(xf), B * Cg, Cg, n_img, _lib.ptr(table_t), _lib.ptr(wf),
                                                  _lib.ptr(dx), B * Nout, Nout, _lib.ptr(dxp), _lib.ptr(yprev if yp_planes is None else None),
                                                  ysv, ysb, _lib.ptr(yp_planes), act, zr, B, n_in, S, Nout, Cg, _lib.stream_ptr()), what)
            return dx, dxp

        fam = "bwd conv_p3s" if kind == 2 else "bwd conv_p3"
        dx, dxp = dense(img_full, None, 0, None, tag)
        check("planes", fam, dx)
        if img_out:
            rec.same(tag + " image", dxp, to_p3(dx))
        if yimg is not None:
            dx2, _ = dense(img_full, None, 0, yimg, tag + " yprev_planes")
            rec.same(tag + " yprev_planes", dx2, dx)
        if kind == 1:
            dxf, dxpf = dense(img_part, f32_part, R, None, tag + " f32 rows")
            check("f32 rows", "bwd conv_p3 f32r", dxf)
            if img_out:
                rec.same(tag + " f32 rows image", dxpf, to_p3(dxf))
        if rag:
            rr, rp = bs.dev["rag_rows"], bs.dev["rag_pos"]
            L = int(rr.shape[1])
            for yp_planes in ((None, yimg) if yimg is not None else (None,)):
                what = tag + " ragged" + (" yprev_planes" if yp_planes is not None else "")
                dxr = torch.full((n_in, B, Nout), NAN, device=d)
                dxpr = torch.full((nb_out,), 255, dtype=torch.uint8, device=d) if img_out else None
                _check(lib.sh_spiral_conv_bwd_data_p3_rag(_lib.ptr(img_part), _lib.ptr(rr), _lib.ptr(rp), L, _lib.ptr(wf), _lib.ptr(dxr), B * Nout,
                                                          Nout, _lib.ptr(dxpr), _lib.ptr(yprev if yp_planes is None else None), ysv, ysb,
                                                          _lib.ptr(yp_planes), act, zr, B, n_in, S, Nout, Cg, _lib.stream_ptr()), what)
                if yp_planes is None:
                    check("ragged", "bwd conv_p3r", dxr)
                    if img_out:
                        rec.same(what + " image", dxpr, to_p3(dxr))
                    dx_rag = dxr
                else:
                    rec.same(what, dxr, dx_rag)
        if use_grp:
            g_r, g_p, g_o = grp
            for yp_planes in ((None, yimg) if yimg is not None else (None,)):
                what = tag + " grouped" + (" yprev_planes" if yp_planes is not None else "")
                dxg = torch.full((n_in, B, Nout), NAN, device=d)
                dxpg = torch.full((nb_out,), 255, dtype=torch.uint8, device=d) if img_out else None
                _check(lib.sh_spiral_conv_p3_grp(_lib.ptr(img_part), _lib.ptr(g_r), _lib.ptr(g_p), _lib.ptr(g_o), int(g_r.shape[0]), int(g_r.shape[1]),
                                                 _lib.ptr(wf), None, _lib.ptr(dxg), B * Nout, Nout, _lib.ptr(dxpg),
                                                 _lib.ptr(yprev if yp_planes is None else None), ysv, ysb, _lib.ptr(yp_planes), act, zr, 1, B, n_in,
                                                 S, Cg, Nout, _lib.stream_ptr()), what)
                if yp_planes is None:
                    check("grouped", "bwd conv_p3g", dxg)
                    if img_out:
                        rec.same(what + " image", dxpg, to_p3(dxg))
                    dx_grp = dxg
                else:
                    rec.same(what, dxg, dx_grp)


def wgrad_p3_reduced(dp_img, zero_row, x_img, table, B, R, S, cin, cout):
    """dW, dbias of the plane weight gradient, its slabs reduced by the library's own reduction (kind 2)."""
    import ctypes
    lib, d = _lib.load(), table.device
    nb = lib.sh_spiral_conv_bwd_wgt_p3_workspace(B, R, S, cin, cout)
    ws = torch.full((nb // 4,), NAN, dtype=torch.float32, device=d)
    _check(lib.sh_spiral_conv_bwd_wgt_p3(_lib.ptr(dp_img), zero_row, _lib.ptr(x_img), _lib.ptr(table), _lib.ptr(ws), nb, B, R, S, cin, cout,
                                         _lib.stream_ptr()), "sh_spiral_conv_bwd_wgt_p3")
    dW = torch.full((cout, S * cin), NAN, device=d)
    db = torch.full((cout,), NAN, device=d)
    P, I = ctypes.c_void_p, ctypes.c_int
    _check(lib.sh_spiral_conv_bwd_wgt_reduce_multi_kinds(1, arr([ws.data_ptr()], P), arr([dW.data_ptr()], P), arr([db.data_ptr()], P),
                                                         arr([B], I), arr([R], I), arr([S], I), arr([cin], I), arr([cout], I), arr([2], I),
                                                         _lib.stream_ptr()), "sh_spiral_conv_bwd_wgt_reduce_multi_kinds")
    return dW, db, ws


def _wgrad(rec, g, view, table, gen, adversarial):
    lib = _lib.load()
    d = table.device
    name, B, R, n_in, S, Cg, Nout, _ = g
    cin, cout = (Cg, Nout) if view == "wA" else (Nout, Cg)
    from semantichuman_amd import ops
    x = rnd((n_in, B, cin), d, adversarial, gen, batch=2)
    dp = rnd((R, B, cout), d, adversarial, gen, batch=4)
    # the zero row completes an odd unit count; with a single row of one unit pair there is none to spare
    zr = R - 1 if (R * (B // 16)) % 2 else -1
    if zr >= 0:
        dp[zr] = 0
    tl = table.long()
    dp64 = dp.double().reshape(R * B, cout)
    ref = torch.empty((cout, S, cin), dtype=torch.float64, device=d)
    for s in range(S):
        ref[:, s, :] = dp64.t() @ x[tl[:, s]].double().reshape(R * B, cin)
    ref = ref.reshape(cout, S * cin)
    refb = dp64.sum(0)
    _lib.set_f32_mma_mode("exact")
    dWe, dbe = ops.spiral_conv_bwd_wgt(dp, "vm", x, "vm", table, R, S, cin, cout)
    dW, db, _ = wgrad_p3_reduced(to_p3(dp), zr, to_p3(x), table, B, R, S, cin, cout)
    tag = "%s %s%s" % (name, view, " adversarial" if adversarial else "")
    rec.gate(tag + " dW", "wgrad_p3 dW", dW, dWe, ref, 1e-4)
    rec.gate(tag + " dbias", "wgrad_p3 dbias", db, dbe, refb, 1e-4)


def _rejected_calls(g, fs, bs, d):
    """Every plane entry point refuses the point: SH_ERR_UNSUPPORTED, no launch.  Buffers are sized for the point all the same."""
    lib = _lib.load()
    name, B, R, n_in, S, Cg, Nout, _ = g
    out = {}
    n_ext = R + bs.n_extra
    big = lambda rows, C: torch.zeros(rows * max(B, 16) * max(C, 16) * 8 + 4096, dtype=torch.uint8, device=d)   # noqa: E731
    xi, di = big(n_in, Cg), big(n_ext, Cg)
    wf = torch.zeros(max(lib.sh_conv_wfrag3_bytes(S, Cg, Nout), 3072) * 2, dtype=torch.uint8, device=d)
    y = torch.zeros((max(R, n_in), B, Nout), device=d)
    tf, tt = fs.dev["table"], bs.dev["table_t"]
    L = 8
    rr = torch.full((n_in, L), R - 1, dtype=torch.int32, device=d)
    rp = torch.full((n_in, L), -1, dtype=torch.int32, device=d)
    ng = max(R, n_in)
    g_rows = torch.zeros((ng, L), dtype=torch.int32, device=d)
    g_pos = torch.full((ng, L), -1, dtype=torch.int32, device=d)
    g_out = torch.full((ng, 4), -1, dtype=torch.int32, device=d)
    s = _lib.stream_ptr()
    out["fwd"] = lib.sh_spiral_conv_fwd_p3(_lib.ptr(xi), _lib.ptr(tf), _lib.ptr(wf), None, _lib.ptr(y), B * Nout, Nout, None, B, R, S, Cg, Nout,
                                           0, R - 1, s)
    out["bwd"] = lib.sh_spiral_conv_bwd_data_p3(_lib.ptr(di), R - 1, None, 0, 0, 0, _lib.ptr(tt), _lib.ptr(wf), _lib.ptr(y), B * Nout, Nout, None,
                                                None, 0, 0, None, 0, -1, B, n_in, S, Nout, Cg, s)
    out["rag"] = lib.sh_spiral_conv_bwd_data_p3_rag(_lib.ptr(di), _lib.ptr(rr), _lib.ptr(rp), L, _lib.ptr(wf), _lib.ptr(y), B * Nout, Nout, None,
                                                    None, 0, 0, None, 0, -1, B, n_in, S, Nout, Cg, s)
    for bw in (0, 1):
        out["grp%d" % bw] = lib.sh_spiral_conv_p3_grp(_lib.ptr(di if bw else xi), _lib.ptr(g_rows), _lib.ptr(g_pos), _lib.ptr(g_out), ng, L,
                                                      _lib.ptr(wf), None, _lib.ptr(y), B * Nout, Nout, None, None, 0, 0, None, 0, -1, bw, B,
                                                      n_in if bw else R, S, Cg, Nout, s)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=d)
    for view, (cin, cout) in (("wA", (Cg, Nout)), ("wB", (Nout, Cg))):
        if not lib.sh_spiral_conv_bwd_wgt_p3_ok(B, R, S, cin, cout):
            out[view] = lib.sh_spiral_conv_bwd_wgt_p3(_lib.ptr(di), R - 1, _lib.ptr(xi), _lib.ptr(tf), _lib.ptr(ws), ws.numel(), B, R, S, cin, cout, s)
    return out


def _run_point(g, d):
    lib = _lib.load()
    name, B, R, n_in, S, Cg, Nout, _ = g
    rec = _Rec()
    fs, bs = _steps(g, d)
    kind = lib.sh_spiral_conv_p3_kind(B, S, Cg, Nout)
    gen = torch.Generator(device=d)
    gen.manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    p3_0 = lib.sh_p3_launch_count()
    if kind == 0:
        n0 = lib.sh_profile_count()
        rc = _rejected_calls(g, fs, bs, d)
        torch.cuda.synchronize()
        for k, v in rc.items():
            if v != SH_ERR_UNSUPPORTED:
                rec.fail.append(("%s rejected %s" % (name, k), "status %d, want SH_ERR_UNSUPPORTED" % v))
        if lib.sh_profile_count() != n0 or lib.sh_p3_launch_count() != p3_0:
            rec.fail.append((name + " rejected", "a refused call launched a kernel"))
    else:
        # list lengths past what the list kernels take are refused without a launch
        n0 = lib.sh_profile_count()
        for key, ok in (("rag", bs.rag is not None), ("grp", fs.fgrp is not None)):
            if not ok:
                continue
            L = 65
            lib_ok = (lib.sh_spiral_conv_p3_rag_ok if key == "rag" else lib.sh_spiral_conv_p3_grp_ok)(B, S, Cg, Nout, L)
            if lib_ok:
                rec.fail.append((name, "%s predicate takes lists of %d" % (key, L)))
                continue
            rows = torch.full((n_in, L), R - 1, dtype=torch.int32, device=d)
            pos = torch.full((n_in, L), -1, dtype=torch.int32, device=d)
            out4 = torch.full((n_in, 4), -1, dtype=torch.int32, device=d)
            buf = torch.zeros(lib.sh_p3_bytes(R + bs.n_extra, B, Cg) + lib.sh_p3_bytes(n_in, B, Cg), dtype=torch.uint8, device=d)
            wf = torch.zeros(lib.sh_conv_wfrag3_bytes(S, Cg, Nout), dtype=torch.uint8, device=d)
            y = torch.zeros((max(R, n_in), B, Nout), device=d)
            if key == "rag":
                rc = lib.sh_spiral_conv_bwd_data_p3_rag(_lib.ptr(buf), _lib.ptr(rows), _lib.ptr(pos), L, _lib.ptr(wf), _lib.ptr(y), B * Nout, Nout,
                                                        None, None, 0, 0, None, 0, -1, B, n_in, S, Nout, Cg, _lib.stream_ptr())
            else:
                rc = lib.sh_spiral_conv_p3_grp(_lib.ptr(buf), _lib.ptr(rows), _lib.ptr(pos), _lib.ptr(out4), n_in, L, _lib.ptr(wf), None, _lib.ptr(y),
                                               B * Nout, Nout, None, None, 0, 0, None, 0, -1, 0, B, R, S, Cg, Nout, _lib.stream_ptr())
            if rc != SH_ERR_UNSUPPORTED:
                rec.fail.append((name, "%s with lists of %d: status %d" % (key, L, rc)))
        torch.cuda.synchronize()
        if lib.sh_profile_count() != n0 or lib.sh_p3_launch_count() != p3_0:
            rec.fail.append((name, "a refused list call launched a kernel"))
        for adversarial in (False, True):
            # forward: layer Cg -> Nout
            w = rnd((Nout, S * Cg), d, True, gen, last=4) if adversarial else (torch.randn((Nout, S * Cg), device=d, generator=gen) / (S * Cg) ** 0.5).contiguous()
            bias = torch.randn((Nout,), device=d, generator=gen).contiguous()
            x = rnd((n_in, B, Cg), d, adversarial, gen, batch=2)
            _fwd(rec, g, fs, w, bias, x, wfrag3(w, S, Cg, Nout, False))
            del x
            # backward-data: layer Nout -> Cg
            wb = rnd((Cg, S * Nout), d, True, gen, last=4) if adversarial else (torch.randn((Cg, S * Nout), device=d, generator=gen) / (S * Nout) ** 0.5).contiguous()
            dp = rnd((R + bs.n_extra, B, Cg), d, adversarial, gen, batch=2)
            dp[R - 1] = 0
            dp[R:] = 0
            from semantichuman_amd import ops
            n1, n2 = bs.tt.n1, bs.tt.n2
            if n1:
                ops.spmm(bs.dev["sum1"], dp, "vm", dp[R:], "vm", n1)
            if n2:
                ops.spmm(bs.dev["sum2"], dp, "vm", dp[R + n1:], "vm", n2)
            z = torch.randn((n_in, B, Nout), device=d, generator=gen)
            yprev = {a: ACT64[a](z.double()).float().contiguous() for a in range(1, 6)}
            _bwd(rec, g, bs, wb, dp, yprev, wfrag3(wb, S, Nout, Cg, True))
            del dp, yprev, z
        if lib.sh_p3_launch_count() == p3_0:
            rec.fail.append((name, "no plane kernel launched"))
    for view, (cin, cout) in (("wA", (Cg, Nout)), ("wB", (Nout, Cg))):
        if lib.sh_spiral_conv_bwd_wgt_p3_ok(B, R, S, cin, cout):
            for adversarial in (False, True):
                _wgrad(rec, g, view, fs.dev["table"], gen, adversarial)
    return rec


@pytest.fixture(scope="module")
def sweep():
    """Runs every grid point once (a point's failure is recorded, not raised) with the profiler on; -> ({name: _Rec}, kernel names)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    d = torch.device("cuda:0")
    was = _lib.get_f32_mma_mode()
    out, names = {}, set()
    try:
        for g in GRID:
            _lib.profile_enable(True)
            try:
                out[g[0]] = _run_point(g, d)
            except Exception as e:                        # noqa: BLE001 - recorded as that point's failure
                rec = _Rec()
                rec.fail.append((g[0], "%s: %s" % (type(e).__name__, e)))
                out[g[0]] = rec
            torch.cuda.synchronize()
            names |= {n for n, _, _ in _lib.profile_records_by_kernel()}
            _lib.profile_enable(False)
    finally:
        _lib.set_f32_mma_mode(was)
    return out, names


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_point_against_float64(sweep, name):
    rec = sweep[0][name]
    assert not rec.fail, rec.fail[:12]


def _reachable_conv_p3():
    """conv_p3_kernel<NT, RT, C16, BWD, NP, F32R> at default settings (choose_p3 / p3_launch_choice, SH_P3_NP = 6)."""
    out = set()
    for c16, nts in ((True, (1, 2)), (False, (1, 2, 4, 8))):
        for nt in nts:
            for rt in ((1,) if nt == 8 else (1, 2)):
                for bwd, f32r in ((False, False), (True, False), (True, True)):
                    out.add("conv_p3_kernel<%d, %d, %s, %s, 6, %s>" % (nt, rt, str(c16).lower(), str(bwd).lower(), str(f32r).lower()))
    return out


@pytest.mark.gpu
def test_sweep_covers_every_reachable_instantiation(sweep):
    recs, names = sweep
    want = _reachable_conv_p3()
    want |= {"conv_p3s_kernel<2, %s, 6, %d>" % (b, nt) for b in ("false", "true") for nt in (2, 4)}
    want |= {"conv_p3r_kernel<%d, 6>" % nt for nt in (1, 2, 4)}
    want |= {"conv_p3g_kernel<%d, %d, %s, 6, false>" % (nt, gg, b) for nt, gg in ((1, 4), (2, 4), (4, 2)) for b in ("false", "true")}
    want |= {"conv_p3g_kernel<%d, 4, %s, 6, true>" % (nt, b) for nt in (1, 2) for b in ("false", "true")}
    missing = sorted(want - names)
    assert not missing, missing
    wp = {n for n in names if n.startswith("wgrad_p3_kernel<")}
    parts = [n[len("wgrad_p3_kernel<"):-1].split(", ") for n in wp]
    assert {p[1] for p in parts} == {"2", "4"}, sorted(wp)
    assert {(p[1], p[2]) for p in parts} >= {("2", "true"), ("4", "true"), ("2", "false"), ("4", "false")}, sorted(wp)
    assert len({p[0] for p in parts}) >= 3, sorted(wp)
    # the numbers behind the gate, per kernel family (worst err_p3 / err_exact and how many checks)
    fam = {}
    for r in recs.values():
        for k, v in r.ratio.items():
            fam[k] = (max(fam.get(k, (0.0, 0))[0], v), fam.get(k, (0.0, 0))[1] + r.n[k])
    print("P3_SWEEP_SUMMARY " + json.dumps({"families": fam, "points": len(recs), "instantiations": sorted(n for n in names if "p3" in n)}))


# ------------------------------------------------------------------------------------------------------------ plane images
@pytest.mark.gpu
@pytest.mark.parametrize("rows,B,C", [(7, 16, 96), (5, 48, 160), (3, 32, 256), (4, 1024, 32), (2, 1024, 16), (9, 16, 16), (3, 1024, 256)])
def test_plane_image_round_trip(rows, B, C):
    """h + m + l is the tensor, bit for bit, in the documented fragment-major layout (tests/test_p3.py at more widths and batches)."""
    torch.manual_seed(rows * C + B)
    x = torch.randn(rows, B, C) * torch.pow(10.0, 6 * torch.rand(rows, B, C) - 3)
    x[0, 0, :4] = torch.tensor([0.0, -0.0, 1.0, -1.0e-30])
    img = to_p3(x.cuda())
    torch.cuda.synchronize()
    assert torch.equal(decode_image(img, rows, B, C), x)


# ------------------------------------------------------------------------------------------- the pre-sum job at another shape
@pytest.mark.gpu
def test_wgrad_presum_job_at_unshipped_shape():
    """sh_spiral_conv_bwd_wgt_p3_presum (default SH_WP3_TAIL): its rows and their image are sh_spmm's, bit for bit, and its slabs
    are those of the launch without a job - at a 32 -> 96 layer, S = 12, B = 80 (two channel tiles per wave)."""
    from semantichuman_amd import ops
    lib = _lib.load()
    d = torch.device("cuda:0")
    torch.manual_seed(12)
    B, R, n_in, S, cin, cout, n_sum = 80, 150, 170, 12, 32, 96, 97
    assert lib.sh_spiral_conv_bwd_wgt_p3_ok(B, R, S, cin, cout)
    table = torch.randint(0, n_in, (R, S), dtype=torch.int32, device=d)
    x = torch.randn(n_in, B, cin, device=d)
    dp = torch.randn(R + n_sum, B, cout, device=d)
    g = np.random.RandomState(2)
    rowptr = np.concatenate([[0], np.cumsum(g.randint(1, 9, size=n_sum))]).astype(np.int32)
    col = g.randint(0, R, size=rowptr[-1]).astype(np.int32)
    m = tuple(torch.from_numpy(a).to(d) for a in (rowptr, col, np.ones(rowptr[-1], dtype=np.float32)))
    xi, di = to_p3(x), to_p3(dp[:R].contiguous())
    nb = lib.sh_spiral_conv_bwd_wgt_p3_workspace(B, R, S, cin, cout)
    ws0 = torch.zeros(nb // 4, device=d)
    _check(lib.sh_spiral_conv_bwd_wgt_p3(_lib.ptr(di), -1, _lib.ptr(xi), _lib.ptr(table), _lib.ptr(ws0), nb, B, R, S, cin, cout, _lib.stream_ptr()), "p3")
    want = dp.clone()
    ops.spmm(m, want, "vm", want[R:], "vm", n_sum)
    got = dp.clone()
    got[R:] = NAN
    img = torch.full((lib.sh_p3_bytes(n_sum, B, cout),), 255, dtype=torch.uint8, device=d)
    ws1 = torch.full_like(ws0, NAN)
    _check(lib.sh_spiral_conv_bwd_wgt_p3_presum(_lib.ptr(di), -1, _lib.ptr(xi), _lib.ptr(table), _lib.ptr(ws1), nb, _lib.ptr(got), B * cout, cout,
                                                _lib.ptr(m[0]), _lib.ptr(m[1]), _lib.ptr(m[2]), _lib.ptr(got[R:]), _lib.ptr(img), n_sum, B, R, S, cin,
                                                cout, _lib.stream_ptr()), "p3_presum")
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(img, to_p3(want[R:].contiguous()))
    assert torch.equal(ws1, ws0)


# ------------------------------------------------------------------------------ whole training steps at unshipped filters
# one training step (forward, L1 + 1e-2 x edge-ratio loss, backward) in a child process with the arenas poisoned with NaN
# (SH_DEBUG_POISON=1); argv = template, batch, FE, FD, latent size, spiral lengths per level, form, output file
_STEP = r"""
import json, sys
import numpy as np, torch
import semantichuman_amd as sh
from semantichuman_amd import _lib, synthetic
from semantichuman_amd.hierarchy import load_hierarchy
tpl, B, fe, fd, nz, ss, form, out = sys.argv[1], int(sys.argv[2]), json.loads(sys.argv[3]), json.loads(sys.argv[4]), int(sys.argv[5]), json.loads(sys.argv[6]), sys.argv[7], sys.argv[8]
dev = torch.device("cuda:0")
h = load_hierarchy(tpl)
spirals = [np.ascontiguousarray(s[:, :k]) for s, k in zip(h.spirals, ss)]
_lib.set_f32_mma_mode(form)
torch.manual_seed(11)
m = sh.SpiralAutoencoder(fe, fd, nz, h.sizes, list(ss), spirals, h.D, h.U, dev)
sd = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
x = torch.from_numpy(synthetic.synth_batch(h.verts, B, seed=4)).to(dev)
ft = sh.FaceTables(h.faces, h.sizes[0] + 1, dev)
n0 = _lib.load().sh_p3_launch_count()
x_hat, z = m(x)
loss = sh.l1_loss(x, x_hat) + 1e-2 * sh.edge_ratio_loss(x_hat, x, ft)
loss.backward()
torch.cuda.synchronize()
res = {"loss": loss.detach().cpu().numpy(), "x_hat": x_hat.detach().cpu().numpy(), "x": x.cpu().numpy(),
       "p3_launches": np.int64(_lib.load().sh_p3_launch_count() - n0)}
res.update({"grad." + n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()})
res.update({"sd." + k: v for k, v in sd.items()})
np.savez(out, **res)
"""

STEP_CONFIGS = [
    # encoder 32 / 64 / 96 / 128, spirals 9 / 9 / 7 / 7 / 5, batch 80
    ("template6890.npz", 80, [[3, 32, 64, 96, 128], [[], [], [], [], []]], [[128, 96, 64, 32, 32], [[], [], [], [], 3]], 64, [9, 9, 7, 7, 5]),
    # 48- and 160-channel levels, spirals 10 / 6 / 8 / 3 / 8, batch 16
    ("template6890.npz", 16, [[3, 16, 48, 160, 64], [[], [], [], [], []]], [[64, 160, 48, 32, 16], [[], [], [], [], 3]], 32, [10, 6, 8, 3, 8]),
]


def _child_step(tmp_path, cfg, form):
    tpl, B, fe, fd, nz, ss = cfg
    out = str(tmp_path / ("%s_%d_%s.npz" % (tpl.split(".")[0], B, form)))
    r = subprocess.run([sys.executable, "-c", _STEP, os.path.join(ROOT, "tests", "golden", tpl), str(B), json.dumps(fe), json.dumps(fd), str(nz),
                        json.dumps(ss), form, out], env=dict(os.environ, SH_DEBUG_POISON="1"), capture_output=True, text=True, timeout=900,
                       cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return dict(np.load(out))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", STEP_CONFIGS, ids=["enc32-64-96-128_S9_B80", "lvl48-160_B16"])
def test_training_step_at_unshipped_filters_against_float64(tmp_path, cfg):
    """One planes3 and one exact training step against oracle/ref_cpu.SpiralAEOracle in float64 (evaluated on the device): loss and
    reconstruction within 1e-5, every parameter gradient within 1e-4 of the largest magnitude.  Catches what both forms would share
    (host tables, plan choices), which the planes3-vs-exact comparisons cannot."""
    from oracle import ref_cpu
    from semantichuman_amd.hierarchy import load_hierarchy
    tpl, B, fe, fd, nz, ss = cfg
    d = torch.device("cuda:0")
    h = load_hierarchy(os.path.join(ROOT, "tests", "golden", tpl))
    res = {form: _child_step(tmp_path, cfg, form) for form in ("exact", "planes3")}
    assert res["planes3"]["p3_launches"] > 0 and res["exact"]["p3_launches"] == 0
    S = [torch.from_numpy(np.ascontiguousarray(s[:, :k]).astype(np.int64))[None].to(d) for s, k in zip(h.spirals, ss)]
    _, D, U = h.dense_constants()
    om = ref_cpu.SpiralAEOracle(fe, fd, nz, h.sizes, list(ss), S, [m.double().to(d) for m in D], [m.double().to(d) for m in U]).double().to(d)
    sd = res["exact"]
    om.load_state_dict({k[3:]: torch.from_numpy(sd[k]).double() for k in sd if k.startswith("sd.")})
    x = torch.from_numpy(res["exact"]["x"]).double().to(d)
    xo, _ = om(x)
    lo = torch.nn.functional.l1_loss(x, xo) + 1e-2 * ref_cpu.edge_ratio_loss(xo, x, torch.as_tensor(h.faces, dtype=torch.long, device=d))
    lo.backward()
    ref = {"loss": lo.detach(), "x_hat": xo.detach()}
    ref.update({"grad." + n: p.grad for n, p in om.named_parameters()})
    bad = []
    for form, got in res.items():
        for k, v in ref.items():
            v = v.cpu().numpy()
            g = got[k]
            tol = 1e-4 if k.startswith("grad.") else 1e-5
            err, scale = float(np.abs(g.astype(np.float64) - v).max()), float(np.abs(v).max())
            if not (np.isfinite(g).all() and err <= tol * scale + 1e-30):
                bad.append((form, k, err, scale))
    assert not bad, bad
