"""Which kernel a three-plane convolution call launches, with which grid, and that the result is right - one row per choice that
choose_p3 (csrc/p3_conv.hip) can make: the resident form at 1 / 2 / 4 / 8 channel tiles per workgroup and at 16
gathered channels, one- and two-row tiles, fp32 rows; the streamed form at two and four tiles; ragged lists; grouped lists of four
and two members - and one row per LDS bracket of the grid routine the bf16 convolutions share with them (sh_resident_grid).

Every row pins the launches of one call as the dispatch record writes them: kernel name with its template arguments, and the
shape tag with the grid (those of the MI355X's 256 CUs).  They were recorded before the choice moved into one routine: a row that
fails says the choice, the grid or the record name moved (the benchmark's tables and the committed profiles read these names).
The three-plane results are held to a float64 gather-matmul under the gate of tests/test_p3_shapes.py (the exact fp32 kernel next
to them), the bf16 ones under that of tests/test_bf16.py (one bf16 ulp at the tensor's scale)."""
import functools

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, mesh_ops, ops
from tests import emulate
from tests.launch_record import launches
from tests.p3_ref import rnd, to_p3, wfrag3
from tests.test_p3_shapes import GRID, _Rec, _steps

pytestmark = pytest.mark.gpu
POINTS = {g[0]: g for g in GRID}


def p3(inst, R, B, K, N, grid, f32=1):
    return ("conv_p3_kernel<%s>" % inst, "R=%d B=%d K=%d N=%d grid=%s f32=%d" % (R, B, K, N, grid, f32))


def p3s(inst, R, B, K, N, grid):
    return ("conv_p3s_kernel<%s>" % inst, "R=%d B=%d K=%d N=%d grid=%s f32=1" % (R, B, K, N, grid))


def p3r(inst, R, B, K, N, grid, L):
    return ("conv_p3r_kernel<%s>" % inst, "R=%d B=%d K=%d N=%d grid=%s L=%d f32=1" % (R, B, K, N, grid, L))


def p3g(inst, R, B, K, N, grid, groups, L):
    return ("conv_p3g_kernel<%s>" % inst, "R=%d B=%d K=%d N=%d grid=%s groups=%d L=%d f32=1" % (R, B, K, N, grid, groups, L))


# (row, grid point of tests/test_p3_shapes.py, call) -> the launch
ROWS = [
    # ---- resident weight <NT, RT, C16, BWD, NP, F32R>
    ("res-nt1-fwd", "s12_c32_n12", "fwd", p3("1, 1, false, false, 6, false", 110, 16, 384, 12, "32x256")),
    ("res-nt1-bwd", "s12_c32_n12", "bwd", p3("1, 1, false, true, 6, false", 110, 16, 384, 12, "32x256")),
    ("res-nt2-fwd", "s3_c128_n32", "fwd", p3("2, 1, false, false, 6, false", 120, 64, 384, 32, "120x256")),
    ("res-nt2-bwd", "s3_c128_n32", "bwd", p3("2, 1, false, true, 6, false", 120, 64, 384, 32, "120x256")),
    ("res-nt4-fwd", "s4_c96_n64", "fwd", p3("4, 1, false, false, 6, false", 100, 64, 384, 64, "104x256")),
    ("res-nt4-bwd", "s4_c96_n64", "bwd", p3("4, 1, false, true, 6, false", 120, 64, 384, 64, "120x256")),
    ("res-nt8-fwd", "s3_c32_n128", "fwd", p3("8, 1, false, false, 6, false", 100, 80, 96, 128, "128x256")),
    ("res-nt8-bwd", "s3_c32_n128", "bwd", p3("8, 1, false, true, 6, false", 140, 80, 96, 128, "176x256")),
    ("res-c16-nt1-fwd", "c16_s3_n12", "fwd", p3("1, 1, true, false, 6, false", 120, 48, 48, 12, "96x256")),
    ("res-c16-nt1-bwd", "c16_s3_n12", "bwd", p3("1, 1, true, true, 6, false", 100, 48, 48, 12, "80x256")),
    ("res-c16-nt2-fwd", "c16_s9_n32", "fwd", p3("2, 1, true, false, 6, false", 77, 64, 144, 32, "80x256")),
    ("res-c16-nt2-bwd", "c16_s9_n32", "bwd", p3("2, 1, true, true, 6, false", 77, 64, 144, 32, "80x256")),
    # two-row tiles from R * B / 16 >= 16 384 (odd R: the last tile is half empty)
    ("res-rt2-fwd", "rt2_c32_n16", "fwd", p3("1, 2, false, false, 6, false", 257, 1024, 128, 16, "1024x256")),
    ("res-rt2-bwd", "rt2_c32_n16", "bwd", p3("1, 2, false, true, 6, false", 300, 1024, 128, 16, "1024x256")),
    ("res-rt2-c16-fwd", "rt2_c16_n32", "fwd", p3("2, 2, true, false, 6, false", 257, 1024, 144, 32, "1024x256")),
    # rows behind the imaged ones read as fp32
    ("res-f32-rows", "s3_c128_n32", "bwd_f32", p3("2, 1, false, true, 6, true", 120, 64, 384, 32, "120x256")),
    # ---- streamed weight <RT, BWD, NP, NT>
    ("str-nt2-fwd", "str_s9_c256_n32", "fwd", p3s("2, false, 6, 2", 71, 16, 2304, 32, "8x512")),
    ("str-nt2-bwd", "str_s9_c256_n32", "bwd", p3s("2, true, 6, 2", 90, 16, 2304, 32, "8x512")),
    ("str-nt4-fwd", "str_s12_c64_n64", "fwd", p3s("2, false, 6, 4", 150, 64, 768, 64, "40x512")),
    ("str-nt4-bwd", "str_s12_c64_n64", "bwd", p3s("2, true, 6, 4", 150, 64, 768, 64, "40x512")),
    # ---- ragged lists <NT, NP>
    ("rag-nt1", "s12_c32_n12", "rag", p3r("1, 6", 110, 16, 384, 12, "32x256", 19)),
    ("rag-nt2", "s3_c128_n32", "rag", p3r("2, 6", 120, 64, 384, 32, "120x256", 6)),
    ("rag-nt4", "s4_c96_n64", "rag", p3r("4, 6", 120, 64, 384, 64, "120x256", 7)),
    # ---- grouped lists <NT, G, BWD, NP, C16>
    ("grp-1x4-fwd", "s12_c32_n12", "fgrp", p3g("1, 4, false, 6, false", 110, 16, 384, 12, "8x256", 29, 30)),
    ("grp-1x4-bwd", "s12_c32_n12", "bgrp", p3g("1, 4, true, 6, false", 110, 16, 384, 12, "8x256", 30, 35)),
    ("grp-2x4-fwd", "s3_c128_n32", "fgrp", p3g("2, 4, false, 6, false", 120, 64, 384, 32, "40x256", 36, 9)),
    ("grp-2x4-bwd", "s3_c128_n32", "bgrp", p3g("2, 4, true, 6, false", 120, 64, 384, 32, "56x256", 49, 12)),
    ("grp-4x2-fwd", "s4_c96_n64", "fgrp", p3g("4, 2, false, 6, false", 100, 64, 384, 64, "56x256", 52, 7)),
    ("grp-4x2-bwd", "s4_c96_n64", "bgrp", p3g("4, 2, true, 6, false", 120, 64, 384, 64, "72x256", 69, 9)),
    ("grp-c16-1x4-fwd", "c16_s3_n12", "fgrp", p3g("1, 4, false, 6, true", 120, 48, 48, 12, "32x256", 33, 9)),
    ("grp-c16-1x4-bwd", "c16_s3_n12", "bgrp", p3g("1, 4, true, 6, true", 100, 48, 48, 12, "32x256", 34, 13)),
    ("grp-c16-2x4-fwd", "c16_s9_n32", "fgrp", p3g("2, 4, false, 6, true", 77, 64, 144, 32, "24x256", 20, 26)),
    ("grp-c16-2x4-bwd", "c16_s9_n32", "bgrp", p3g("2, 4, true, 6, true", 77, 64, 144, 32, "24x256", 22, 24)),
]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Operands of a grid point, the float64 results and the exact kernels' (computed once per point, shared by its rows)."""
    g = POINTS[name]
    _, B, R, n_in, S, Cg, Nout, _ = g
    d = torch.device("cuda:0")
    fs, bs = _steps(g, d)
    gen = torch.Generator(device=d)
    gen.manual_seed(R * 131 + S)
    c = dict(g=g, fs=fs, bs=bs)
    was = _lib.get_f32_mma_mode()
    _lib.set_f32_mma_mode("exact")
    try:
        # forward: the layer Cg -> Nout, dummy row R - 1
        w = (torch.randn((Nout, S * Cg), device=d, generator=gen) / (S * Cg) ** 0.5).contiguous()
        bias = torch.randn((Nout,), device=d, generator=gen).contiguous()
        x = rnd((n_in, B, Cg), d, False, gen)
        tl, w64 = fs.dev["table"].long(), w.double().view(Nout, S, Cg)
        ref = torch.zeros((R, B, Nout), dtype=torch.float64, device=d)
        for s in range(S):
            ref += x[tl[:, s]].double() @ w64[:, s, :].t()
        ref += bias.double()
        ref[R - 1] = 0
        ye = torch.full((R, B, Nout), float("nan"), device=d)
        ops.spiral_conv_fwd(x, "vm", fs.dev["table"], w, bias, ye, "vm", R, S, 0, R - 1)
        c.update(xp=to_p3(x), wf=wfrag3(w, S, Cg, Nout, False), bias=bias, fwd_ref=ref, fwd_exact=ye)
        # backward-data: the layer Nout -> Cg over the same table; pre-summed rows behind the R real ones
        wb = (torch.randn((Cg, S * Nout), device=d, generator=gen) / (S * Nout) ** 0.5).contiguous()
        dp = rnd((R + bs.n_extra, B, Cg), d, False, gen)
        dp[R - 1:] = 0
        n1, n2 = bs.tt.n1, bs.tt.n2
        if n1:
            ops.spmm(bs.dev["sum1"], dp, "vm", dp[R:], "vm", n1)
        if n2:
            ops.spmm(bs.dev["sum2"], dp, "vm", dp[R + n1:], "vm", n2)
        w64 = wb.double().view(Cg, S, Nout)
        ref = torch.zeros((n_in, B, Nout), dtype=torch.float64, device=d)
        for s in range(S):
            ref.index_add_(0, tl[:, s], dp[:R].double() @ w64[:, s, :])
        ref[n_in - 1] = 0                                       # the dummy input row's gradient is dropped
        de = torch.full((n_in, B, Nout), float("nan"), device=d)
        ops.spiral_conv_bwd_data(dp, "vm", bs.dev["table_t"], ops.weight_transpose(wb, S, Nout, Cg), de, "vm", None, "vm", 0, -1, n_in, S, Nout, Cg)
        img_part = to_p3(dp[:R].contiguous(), rows=R + bs.n_extra)
        img_part[_lib.load().sh_p3_bytes(R, B, Cg):] = 255      # rows without an image: NaN in the image, and in the fp32 rows below R
        f32_part = dp.clone()
        f32_part[:R] = float("nan")
        c.update(img_full=to_p3(dp), img_part=img_part, f32_part=f32_part, wft=wfrag3(wb, S, Nout, Cg, True), bwd_ref=ref, bwd_exact=de)
    finally:
        _lib.set_f32_mma_mode(was)
    return c


def run_row(name, call):
    """-> (the launches of the row's one call, its result, the exact kernel's, float64, the gate's tolerance on the exact kernel)"""
    lib, P, st = _lib.load(), _lib.ptr, _lib.stream_ptr
    c = _case(name)
    _, B, R, n_in, S, Cg, Nout, _ = c["g"]
    fwd = call in ("fwd", "fgrp")
    rows = R if fwd else n_in
    y = torch.full((rows, B, Nout), float("nan"), device=c["xp"].device)
    if call == "fwd":
        fn = lambda: lib.sh_spiral_conv_fwd_p3(P(c["xp"]), P(c["fs"].dev["table"]), P(c["wf"]), P(c["bias"]), P(y), B * Nout, Nout, None, B, R, S, Cg,   # noqa: E731
                                               Nout, 0, R - 1, st())
    elif call == "fgrp":
        g_r, g_p, g_o = c["fs"].dev["fgrp"]
        fn = lambda: lib.sh_spiral_conv_p3_grp(P(c["xp"]), P(g_r), P(g_p), P(g_o), int(g_r.shape[0]), int(g_r.shape[1]), P(c["wf"]), P(c["bias"]),   # noqa: E731
                                               P(y), B * Nout, Nout, None, None, 0, 0, None, 0, R - 1, 0, B, R, S, Cg, Nout, st())
    elif call in ("bwd", "bwd_f32"):
        xp, xf, n_img = (c["img_full"], None, 0) if call == "bwd" else (c["img_part"], c["f32_part"], R)
        fn = lambda: lib.sh_spiral_conv_bwd_data_p3(P(xp), R - 1, P(xf), B * Cg, Cg, n_img, P(c["bs"].dev["table_t"]), P(c["wft"]), P(y), B * Nout,   # noqa: E731
                                                    Nout, None, None, 0, 0, None, 0, -1, B, n_in, S, Nout, Cg, st())
    elif call == "rag":
        rr, rp = c["bs"].dev["rag_rows"], c["bs"].dev["rag_pos"]
        fn = lambda: lib.sh_spiral_conv_bwd_data_p3_rag(P(c["img_part"]), P(rr), P(rp), int(rr.shape[1]), P(c["wft"]), P(y), B * Nout, Nout, None,   # noqa: E731
                                                        None, 0, 0, None, 0, -1, B, n_in, S, Nout, Cg, st())
    else:
        g_r, g_p, g_o = c["bs"].dev["bgrp"]
        fn = lambda: lib.sh_spiral_conv_p3_grp(P(c["img_part"]), P(g_r), P(g_p), P(g_o), int(g_r.shape[0]), int(g_r.shape[1]), P(c["wft"]), None,   # noqa: E731
                                               P(y), B * Nout, Nout, None, None, 0, 0, None, 0, -1, 1, B, n_in, S, Cg, Nout, st())
    rc, rec = launches(fn)
    _lib.check(rc, "%s %s" % (name, call))
    return rec, y, c["fwd_exact" if fwd else "bwd_exact"], c["fwd_ref" if fwd else "bwd_ref"], 1e-5 if fwd else 1e-4


@pytest.mark.parametrize("name, call, expect", [pytest.param(n, c, e, id=i) for i, n, c, e in ROWS])
def test_p3_form(name, call, expect):
    rec, y, exact, ref, tol = run_row(name, call)
    print("launches:", rec)
    assert rec == [expect]
    gate = _Rec()
    gate.gate("%s %s" % (name, call), call, y, exact, ref, tol)
    assert not gate.fail, gate.fail


# ------------------------------------------------------------------------------------------------ the bf16 convolutions' grids
def bc(inst, R, B, S, Cg, N, grid):
    return ("conv_bf16_kernel<%s>" % inst, "R=%d B=%d S=%d Cg=%d N=%d grid=%s" % (R, B, S, Cg, N, grid))


# (row, (B, n_in, R, S, Cin, Cout), ragged) -> the launch; the resident weight takes nks x NT KiB of LDS.  (With so few work items
# every bracket ends at four waves per workgroup and one workgroup per four items, rounded up to eight: the rows pin that these
# launchers size their grids by the shared routine; the brackets' own caps bind from ~2000 items on - the benchmark's shapes.)
BF16_ROWS = [
    ("bc-lds-10k", (16, 50, 50, 9, 16, 32), False, bc("2, 2, 1, false, false", 50, 16, 9, 16, 32, "8x256")),            # <= 36 KiB: four workgroups per CU
    ("bc-lds-64k", (16, 40, 40, 8, 64, 64), False, bc("4, 1, 4, false, false", 40, 16, 8, 64, 64, "16x256")),            # <= 76 KiB: two
    ("bc-lds-128k", (20, 33, 33, 8, 64, 128), False, bc("8, 1, 4, false, false", 33, 20, 8, 64, 128, "24x256")),          # above: one
    ("bcr", (16, 40, 40, 8, 64, 64), True, ("conv_bf16r_kernel<4>", "R=40 B=16 S=8 Cg=64 N=64 grid=16x256 L=12")),
]


def run_bf16_row(shape, ragged):
    """-> (the launches of the row's one call, its result, float64 on the same bf16-rounded operands), as tests/test_bf16.py"""
    B, n_in, R, S, Cin, Cout = shape
    d = torch.device("cuda:0")
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)          # noqa: E731
    torch.manual_seed(S * Cin + Cout)
    g = np.random.RandomState(1)
    table = g.randint(0, n_in, size=(R, S)).astype(np.int32)
    table[:, 0] = np.arange(R) % n_in
    table[g.rand(R, S) < 0.1] = n_in - 1
    W = bf(torch.randn(Cout, S * Cin) / np.sqrt(S * Cin))
    wf, wft = ops.conv_wfrag_prep([W.to(d)] * 2, [(S, Cin, Cout)] * 2, [0, 1])
    if not ragged:
        x = bf(torch.randn(n_in, B, Cin))
        x[-1] = 0.0
        bias = torch.randn(Cout) * 0.1
        ref = emulate.conv_fwd(x.double().numpy(), table, W.double().numpy(), bias.double().numpy(), 0, R - 1)
        y = torch.full((R, B, Cout), float("nan"), dtype=torch.bfloat16, device=d)
        xd, td, bd = x.to(d, torch.bfloat16), torch.from_numpy(table).to(d), bias.to(d)
        _, rec = launches(lambda: ops.spiral_conv_fwd_bf16(xd, "vm", td, wf, bd, y, "vm", R, S, Cin, Cout, 0, R - 1))
        return rec, y, ref
    tt = mesh_ops.transpose_table_dense(table, n_in, none_row=R - 1, skip_row=-1)
    rag = mesh_ops.transpose_table_ragged(table, n_in, none_row=R - 1, skip_row=n_in - 1)
    assert ops.spiral_conv_bf16_rag_ok(B, S, Cout, Cin, rag[0].shape[1])
    dpre = bf(torch.randn(R, B, Cout))
    dpre[R - 1] = 0
    ref = emulate.conv_bwd_data(emulate.extend_dpre(dpre.double().numpy(), tt), tt.table_t, W.double().numpy(), Cin)
    ref[n_in - 1] = 0
    dx = torch.full((n_in, B, Cin), float("nan"), dtype=torch.bfloat16, device=d)
    dpd, rr, rp = dpre.to(d, torch.bfloat16), torch.from_numpy(rag[0]).to(d), torch.from_numpy(rag[1]).to(d)
    _, rec = launches(lambda: ops.spiral_conv_bwd_data_bf16_rag(dpd, "vm", rr, rp, wft, dx, "vm", None, "vm", 0, n_in - 1, n_in, S, Cin, Cout))
    return rec, dx, ref


@pytest.mark.parametrize("shape, ragged, expect", [pytest.param(s, r, e, id=i) for i, s, r, e in BF16_ROWS])
def test_bf16_conv_grid(shape, ragged, expect):
    rec, y, ref = run_bf16_row(shape, ragged)
    print("launches:", rec)
    assert rec == [expect]
    got = y.float().cpu().double().numpy()
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    assert np.isfinite(got).all() and err <= 2.0 ** -8 * scale + 1e-6, (err, scale)
