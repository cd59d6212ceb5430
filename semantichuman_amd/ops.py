"""Typed Python wrappers around the C ABI (one function per entry point of sh_kernels.h).

Tensors are fp32, contiguous, on a HIP device.  A 3-D activation has one of two layouts:
    'bm'  batch-major  [B, rows, C]   - the reference layout (models.py:37)
    'vm'  vertex-major [rows, B, C]   - the internal fast layout (a gathered neighbour is one
                                        contiguous B*C block -> coalesced 16-byte reads)
The kernels take explicit strides, so both layouts go through the same code.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import ACT_IDS, check, ptr, stream_ptr


def _dims(t: torch.Tensor, layout: str, dtypes=(torch.float32,)):
    """-> (B, rows, C, stride_row, stride_batch) for a contiguous 3-D tensor."""
    if t.dim() != 3 or not t.is_contiguous() or t.dtype not in dtypes:
        raise ValueError("expected a contiguous %s 3-D tensor, got %s %s" % ("/".join(str(d) for d in dtypes), tuple(t.shape), t.dtype))
    if not t.is_cuda:
        raise RuntimeError("semantichuman_amd kernels need a HIP device tensor (got %s); there is no CPU path" % t.device)
    if layout == "bm":
        B, R, C = t.shape
        return B, R, C, C, R * C
    if layout == "vm":
        R, B, C = t.shape
        return B, R, C, B * C, C
    raise ValueError("layout must be 'bm' or 'vm'")


def _check_index_range(t):
    if t.numel() >= 2 ** 32:
        raise RuntimeError("semantichuman_amd: gathered tensors are addressed with 32-bit element offsets; "
                           "%d elements is too large - split the batch" % t.numel())


def alloc(B: int, rows: int, C: int, layout: str, device, extra_rows: int = 0) -> torch.Tensor:
    if layout == "bm":
        if extra_rows:
            raise ValueError("extra rows need the vertex-major layout")
        return torch.empty((B, rows, C), dtype=torch.float32, device=device)
    return torch.empty((rows + extra_rows, B, C), dtype=torch.float32, device=device)


def act_id(name: str) -> int:
    if name not in ACT_IDS:
        raise NotImplementedError(name)          # same error type as reference models.py:31-32
    return ACT_IDS[name]


def spiral_conv_fwd(x, x_layout, table, weight, bias, y, y_layout, R, S, act, zero_row):
    B, _, Cin, xsv, xsb = _dims(x, x_layout)
    B2, Ry, Cout, ysv, ysb = _dims(y, y_layout)
    assert B == B2 and Ry >= R and weight.shape == (Cout, S * Cin) and table.dtype == torch.int32
    _check_index_range(x)
    check(_lib.load().sh_spiral_conv_fwd(ptr(x), xsv, xsb, ptr(table), ptr(weight), ptr(bias), ptr(y), ysv, ysb,
                                         B, R, S, Cin, Cout, act, zero_row, _lib.mma_id(), stream_ptr()), "sh_spiral_conv_fwd")


def spiral_conv_bwd_data(dpre, dp_layout, table_t, weight_t, dx, dx_layout, yprev, yp_layout, act_prev, zero_row,
                         n_in, S, Cin, Cout):
    B, _, C1, dsv, dsb = _dims(dpre, dp_layout)
    B2, Rx, C2, xsv, xsb = _dims(dx, dx_layout)
    assert B == B2 and C1 == Cout and C2 == Cin and Rx >= n_in and weight_t.shape == (Cin, S * Cout)
    assert table_t.dtype == torch.int32 and tuple(table_t.shape) == (n_in, S)
    _check_index_range(dpre)
    if yprev is not None:
        _, _, C3, ysv, ysb = _dims(yprev, yp_layout)
        assert C3 == Cin
    else:
        ysv = ysb = 0
    check(_lib.load().sh_spiral_conv_bwd_data(ptr(dpre), dsv, dsb, ptr(table_t), ptr(weight_t), ptr(dx), xsv, xsb,
                                              ptr(yprev), ysv, ysb, act_prev, zero_row, B, n_in, S, Cin, Cout,
                                              _lib.mma_id(), stream_ptr()), "sh_spiral_conv_bwd_data")


def weight_transpose(weight, S, Cin, Cout):
    wt = torch.empty((Cin, S * Cout), dtype=torch.float32, device=weight.device)
    check(_lib.load().sh_weight_transpose(ptr(weight), ptr(wt), S, Cin, Cout, stream_ptr()), "sh_weight_transpose")
    return wt


def spiral_conv_bwd_wgt(dpre, dp_layout, x, x_layout, table, R, S, Cin, Cout, want_bias=True):
    B, _, C1, dsv, dsb = _dims(dpre, dp_layout)
    B2, _, C2, xsv, xsb = _dims(x, x_layout)
    assert B == B2 and C1 == Cout and C2 == Cin
    lib = _lib.load()
    nbytes = lib.sh_spiral_conv_bwd_wgt_workspace(B, R, S, Cin, Cout)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    dW = torch.empty((Cout, S * Cin), dtype=torch.float32, device=x.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if want_bias else None
    check(lib.sh_spiral_conv_bwd_wgt(ptr(dpre), dsv, dsb, ptr(x), xsv, xsb, ptr(table), ptr(dW), ptr(db), ptr(ws),
                                     nbytes, B, R, S, Cin, Cout, _lib.mma_id(), stream_ptr()), "sh_spiral_conv_bwd_wgt")
    return dW, db


def spiral_conv_bwd_wgt_deferred(dpre, dp_layout, x, x_layout, table, R, S, Cin, Cout, want_bias=True):
    """Weight-gradient pass that only writes its partial slabs; returns a job for
    `spiral_conv_bwd_wgt_reduce` (which reduces the slabs of a whole stack in one launch)."""
    B, _, C1, dsv, dsb = _dims(dpre, dp_layout)
    B2, _, C2, xsv, xsb = _dims(x, x_layout)
    assert B == B2 and C1 == Cout and C2 == Cin
    lib = _lib.load()
    nbytes = lib.sh_spiral_conv_bwd_wgt_workspace(B, R, S, Cin, Cout)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    check(lib.sh_spiral_conv_bwd_wgt(ptr(dpre), dsv, dsb, ptr(x), xsv, xsb, ptr(table), ptr(None), ptr(None), ptr(ws),
                                     nbytes, B, R, S, Cin, Cout, _lib.mma_id(), stream_ptr()), "sh_spiral_conv_bwd_wgt")
    dW = torch.empty((Cout, S * Cin), dtype=torch.float32, device=x.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if want_bias else None
    return dict(ws=ws, dW=dW, db=db, dims=(B, R, S, Cin, Cout))


def _c_ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[0 if t is None else t.data_ptr() for t in tensors])


def _c_int_array(vals):
    import ctypes
    return (ctypes.c_int * len(vals))(*vals)


def spiral_conv_bwd_wgt_reduce(jobs):
    """One launch: fixed-order reduction of the partial slabs of every job (<= 16)."""
    if not jobs:
        return
    import ctypes
    cols = list(zip(*[j["dims"] for j in jobs]))
    args = [_c_ptr_array([j["ws"] for j in jobs]), _c_ptr_array([j["dW"] for j in jobs]), _c_ptr_array([j["db"] for j in jobs])]
    args += [_c_int_array(c) for c in cols]
    check(_lib.load().sh_spiral_conv_bwd_wgt_reduce_multi(len(jobs), *[ctypes.cast(a, ctypes.c_void_p) for a in args], stream_ptr()),
          "sh_spiral_conv_bwd_wgt_reduce_multi")


def weight_transpose_multi(weights, dims):
    """dims: [(S, Cin, Cout)] -> list of weight_t tensors, one launch."""
    import ctypes
    outs = [torch.empty((ci, s * co), dtype=torch.float32, device=w.device) for w, (s, ci, co) in zip(weights, dims)]
    cols = list(zip(*dims))
    args = [_c_ptr_array(list(weights)), _c_ptr_array(outs)] + [_c_int_array(c) for c in cols]
    check(_lib.load().sh_weight_transpose_multi(len(outs), *[ctypes.cast(a, ctypes.c_void_p) for a in args], stream_ptr()),
          "sh_weight_transpose_multi")
    return outs


def act_backward(dy, dy_layout, y, y_layout, dpre, dp_layout, R, act, zero_row):
    B, _, C, asv, asb = _dims(dy, dy_layout)
    _, _, _, ysv, ysb = _dims(y, y_layout)
    _, _, _, psv, psb = _dims(dpre, dp_layout)
    check(_lib.load().sh_act_backward(ptr(dy), asv, asb, ptr(y), ysv, ysb, ptr(dpre), psv, psb, B, R, C, act, zero_row,
                                      stream_ptr()), "sh_act_backward")


def spmm(csr_dev, x, x_layout, y, y_layout, rows, yprev=None, yp_layout="vm", act_prev=0, zero_row=-1):
    """csr_dev = (rowptr, col, val) device tensors."""
    B, _, C, xsv, xsb = _dims(x, x_layout)
    B2, Ry, C2, ysv, ysb = _dims(y, y_layout)
    assert B == B2 and C == C2 and Ry >= rows
    if yprev is not None:
        _, _, _, psv, psb = _dims(yprev, yp_layout)
    else:
        psv = psb = 0
    rowptr, col, val = csr_dev
    check(_lib.load().sh_spmm(ptr(rowptr), ptr(col), ptr(val), ptr(x), xsv, xsb, ptr(y), ysv, ysb, ptr(yprev), psv, psb,
                              act_prev, zero_row, B, rows, C, stream_ptr()), "sh_spmm")


def _linear_ws(M, N, K, device):
    nbytes = _lib.load().sh_linear_workspace(M, N, K)
    return torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.float32, device=device), nbytes


def _check2d(*ts):
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("semantichuman_amd linear kernels need contiguous fp32 HIP tensors (got %s %s %s); there is "
                               "no CPU path" % (t.device, t.dtype, tuple(t.shape)))


def linear_fwd(x, weight, bias, mma=None):
    """y = x @ weight.T + bias for x [M,K], weight [N,K] (nn.Linear layout).  mma: arithmetic form of the products (None = the
    caller's default, _lib.get_f32_mma_mode())."""
    _check2d(x, weight, bias)
    M, K = x.shape
    N = weight.shape[0]
    assert weight.shape[1] == K
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    ws, nb = _linear_ws(M, N, K, x.device)
    check(_lib.load().sh_linear_fwd(ptr(x), ptr(weight), ptr(bias), ptr(y), M, N, K, ptr(ws), nb, _lib.mma_id(mma), stream_ptr()), "sh_linear_fwd")
    return y


def linear_bwd_data(dy, weight, mma=None):
    _check2d(dy, weight)
    M, N = dy.shape
    K = weight.shape[1]
    dx = torch.empty((M, K), dtype=torch.float32, device=dy.device)
    ws, nb = _linear_ws(M, N, K, dy.device)
    check(_lib.load().sh_linear_bwd_data(ptr(dy), ptr(weight), ptr(dx), M, N, K, ptr(ws), nb, _lib.mma_id(mma), stream_ptr()), "sh_linear_bwd_data")
    return dx


def linear_bwd_wgt(dy, x, want_bias=True, mma=None):
    _check2d(dy, x)
    M, N = dy.shape
    K = x.shape[1]
    dW = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    db = torch.empty((N,), dtype=torch.float32, device=dy.device) if want_bias else None
    ws, nb = _linear_ws(M, N, K, dy.device)
    check(_lib.load().sh_linear_bwd_wgt(ptr(dy), ptr(x), ptr(dW), ptr(db), M, N, K, ptr(ws), nb, _lib.mma_id(mma), stream_ptr()), "sh_linear_bwd_wgt")
    return dW, db


def linear_bwd_wgt_adam_ok(M, N, K):
    return bool(_lib.load().sh_linear_bwd_wgt_adam_ok(int(M), int(N), int(K)))


def linear_bwd_wgt_adam(dy, x, weight, exp_avg, exp_avg_sq, step, lr, betas, eps, weight_decay, want_bias=True, mma=None, weight_bf16=None):
    """dW = dy^T x used as the gradient of Adam's update of `weight` / `exp_avg` / `exp_avg_sq`, in place, in the kernel that
    computes it (sh_linear_bwd_wgt_adam); returns the bias gradient (or None).  `step` is not advanced (sh_adam_step with a
    zero-length entry, or sh_adam_bump).  dy / x: fp32 or bf16; `weight_bf16`: the bf16 working copy to rewrite, or None."""
    for t in (dy, x):
        if not (t.is_cuda and t.dim() == 2 and t.is_contiguous() and t.dtype in (torch.float32, torch.bfloat16)):
            raise RuntimeError("linear_bwd_wgt_adam: dy / x must be contiguous 2-D fp32 or bf16 HIP tensors")
    M, N = dy.shape
    K = x.shape[1]
    for t in (weight, exp_avg, exp_avg_sq):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (N, K)):
            raise RuntimeError("linear_bwd_wgt_adam: weight / exp_avg / exp_avg_sq must be contiguous fp32 [%d, %d] HIP tensors" % (N, K))
    if weight_bf16 is not None and not (weight_bf16.dtype == torch.bfloat16 and weight_bf16.is_contiguous() and tuple(weight_bf16.shape) == (N, K)):
        raise RuntimeError("linear_bwd_wgt_adam: the bf16 working copy must be a contiguous bf16 [%d, %d] tensor" % (N, K))
    db = torch.empty((N,), dtype=torch.float32, device=dy.device) if want_bias else None
    did = lambda t: 1 if t.dtype == torch.bfloat16 else 0               # noqa: E731 - enum sh_dtype
    check(_lib.load().sh_linear_bwd_wgt_adam(ptr(dy), did(dy), ptr(x), did(x), ptr(weight), ptr(weight_bf16), ptr(exp_avg), ptr(exp_avg_sq),
                                             ptr(step), ptr(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), ptr(db),
                                             M, N, K, _lib.mma_id(mma), stream_ptr()), "sh_linear_bwd_wgt_adam")
    return db


def _glin_args(x_off, y_off, N, K):
    import ctypes
    G = len(N)
    arr64 = lambda v: (ctypes.c_int64 * G)(*[int(t) for t in v])          # noqa: E731
    arr32 = lambda v: (ctypes.c_int * G)(*[int(t) for t in v])            # noqa: E731
    return G, arr64(x_off), arr64(y_off), arr32(N), arr32(K)


def _ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[0 if t is None else t.data_ptr() for t in tensors])


def grouped_linear_fwd(x, x_off, weights, biases, y_cols, y_off):
    """y[:, y_off[g]:y_off[g]+N_g] = x[:, x_off[g]:x_off[g]+K_g] @ W_g.T + b_g for every group, one launch.
    x [M, Kx] contiguous fp32; weights: list of [N_g, K_g]; biases: list (entries may be None) or None."""
    _check2d(x, *weights)
    M = x.shape[0]
    y = torch.empty((M, y_cols), dtype=torch.float32, device=x.device)
    G, xo, yo, N, K = _glin_args(x_off, y_off, [w.shape[0] for w in weights], [w.shape[1] for w in weights])
    check(_lib.load().sh_grouped_linear_fwd(G, ptr(x), x.shape[1], xo, _ptr_array(weights),
                                            _ptr_array(biases) if biases is not None else None, ptr(y), y_cols, yo, M, N, K,
                                            stream_ptr()), "sh_grouped_linear_fwd")
    return y


def grouped_linear_bwd_data(dy, y_off, weights, x_cols, x_off):
    _check2d(dy, *weights)
    M = dy.shape[0]
    dx = torch.zeros((M, x_cols), dtype=torch.float32, device=dy.device)      # columns no group covers stay zero
    G, xo, yo, N, K = _glin_args(x_off, y_off, [w.shape[0] for w in weights], [w.shape[1] for w in weights])
    check(_lib.load().sh_grouped_linear_bwd_data(G, ptr(dy), dy.shape[1], yo, _ptr_array(weights), ptr(dx), x_cols, xo, M, N, K,
                                                 stream_ptr()), "sh_grouped_linear_bwd_data")
    return dx


def grouped_linear_bwd_wgt(dy, y_off, x, x_off, weights, want_bias):
    _check2d(dy, x)
    M = dy.shape[0]
    dWs = [torch.empty_like(w) for w in weights]
    dbs = [torch.empty((w.shape[0],), dtype=torch.float32, device=w.device) if wb else None for w, wb in zip(weights, want_bias)]
    G, xo, yo, N, K = _glin_args(x_off, y_off, [w.shape[0] for w in weights], [w.shape[1] for w in weights])
    check(_lib.load().sh_grouped_linear_bwd_wgt(G, ptr(dy), dy.shape[1], yo, ptr(x), x.shape[1], xo, _ptr_array(dWs),
                                                _ptr_array(dbs), M, N, K, stream_ptr()), "sh_grouped_linear_bwd_wgt")
    return dWs, dbs


def _ws(device):
    return torch.empty(_lib.load().sh_reduce_workspace() // 4, dtype=torch.float32, device=device)


def l1_loss_fwd(a, b):
    assert a.shape == b.shape and a.is_contiguous() and b.is_contiguous() and a.is_cuda
    out = torch.empty((), dtype=torch.float32, device=a.device)
    check(_lib.load().sh_l1_loss_fwd(ptr(a), ptr(b), a.numel(), ptr(out), ptr(_ws(a.device)), stream_ptr()), "sh_l1_loss_fwd")
    return out


def l1_loss_bwd(a, b, gscale):
    g = torch.empty_like(b)
    check(_lib.load().sh_l1_loss_bwd(ptr(a), ptr(b), a.numel(), ptr(gscale), ptr(g), stream_ptr()), "sh_l1_loss_bwd")
    return g


def vertex_l2(a, b, n_real, scale=1000.0):
    assert a.shape == b.shape and a.dim() == 3 and a.shape[2] == 3 and a.is_contiguous() and b.is_contiguous()
    out = torch.empty((), dtype=torch.float32, device=a.device)
    check(_lib.load().sh_vertex_l2(ptr(a), ptr(b), a.shape[0], a.shape[1], n_real, scale, ptr(out), ptr(_ws(a.device)),
                                   stream_ptr()), "sh_vertex_l2")
    return out


def edge_ratio_loss_fwd(x_hat, x, faces):
    assert x_hat.shape == x.shape and x.shape[2] == 3 and x_hat.is_contiguous() and x.is_contiguous()
    out = torch.empty((), dtype=torch.float32, device=x.device)
    check(_lib.load().sh_edge_ratio_loss_fwd(ptr(x_hat), ptr(x), ptr(faces), x.shape[0], x.shape[1], faces.shape[0], ptr(out),
                                             ptr(_ws(x.device)), stream_ptr()), "sh_edge_ratio_loss_fwd")
    return out


def recon_loss_fwd(x_hat, x, faces, edge_w):
    """-> (total float32 [], parts float32 [2] = (l1, edge)) for contiguous [B, N1, 3] tensors; two separate allocations,
    so that neither is a view autograd would have to copy through."""
    assert x_hat.shape == x.shape and x.shape[2] == 3 and x_hat.is_contiguous() and x.is_contiguous() and x.is_cuda
    total = torch.empty((), dtype=torch.float32, device=x.device)
    parts = torch.empty((2,), dtype=torch.float32, device=x.device)
    ws = torch.empty(_lib.load().sh_recon_loss_workspace() // 4, dtype=torch.float32, device=x.device)
    check(_lib.load().sh_recon_loss_fwd(ptr(x_hat), ptr(x), ptr(faces), x.shape[0], x.shape[1], faces.shape[0], float(edge_w),
                                        ptr(total), ptr(parts), ptr(ws), stream_ptr()), "sh_recon_loss_fwd")
    return total, parts


def recon_loss_bwd(x_hat, x, n_faces, vptr, vnbr, edge_w, gscale):
    g = torch.empty_like(x_hat)
    check(_lib.load().sh_recon_loss_bwd(ptr(x_hat), ptr(x), ptr(vptr), ptr(vnbr), x.shape[0], x.shape[1], int(n_faces),
                                        float(edge_w), ptr(gscale), ptr(g), stream_ptr()), "sh_recon_loss_bwd")
    return g


def edge_ratio_loss_bwd(x_hat, x, faces, vptr, vcorner, gscale):
    g = torch.empty_like(x_hat)
    check(_lib.load().sh_edge_ratio_loss_bwd(ptr(x_hat), ptr(x), ptr(faces), ptr(vptr), ptr(vcorner), x.shape[0], x.shape[1],
                                             faces.shape[0], ptr(gscale), ptr(g), stream_ptr()), "sh_edge_ratio_loss_bwd")
    return g


def measure_girth(v, rings):
    """v [B, rows, 3] fp32 (rows may include the dummy row); rings = (ptr, a, b, f) device tensors -> girth [B, P]."""
    ptr_, a, b, f = rings
    if not (v.is_cuda and v.dtype == torch.float32 and v.dim() == 3 and v.shape[2] == 3 and v.stride(2) == 1
            and v.stride(1) == 3):
        raise RuntimeError("semantichuman_amd.measure_girth needs fp32 HIP vertices [B, rows, 3] (got %s %s %s); there is "
                           "no CPU path" % (v.device, v.dtype, tuple(v.shape)))
    B, P = v.shape[0], ptr_.numel() - 1
    out = torch.empty((B, P), dtype=torch.float32, device=v.device)
    check(_lib.load().sh_measure_girth(ptr(v), v.stride(0) if B > 1 else v.shape[1] * 3, ptr(ptr_), ptr(a), ptr(b), ptr(f),
                                       B, P, ptr(out), stream_ptr()), "sh_measure_girth")
    return out


def bone_length(kps, bones):
    """kps [B, K, 3] fp32 contiguous; bones int32 [P, 3] (third id -1 for a two-joint bone) -> length [B, P]."""
    if not (kps.is_cuda and kps.dtype == torch.float32 and kps.dim() == 3 and kps.shape[2] == 3 and kps.is_contiguous()):
        raise RuntimeError("semantichuman_amd.bone_length needs contiguous fp32 HIP joints [B, K, 3]; there is no CPU path")
    B, K, P = kps.shape[0], kps.shape[1], bones.shape[0]
    out = torch.empty((B, P), dtype=torch.float32, device=kps.device)
    check(_lib.load().sh_bone_length(ptr(kps), ptr(bones), B, K, P, ptr(out), stream_ptr()), "sh_bone_length")
    return out


def measure_girth_bwd(v, rings, g_girth):
    """Gradient of measure_girth w.r.t. v: -> contiguous [B, rows, 3] (rows no ring touches: 0).  rings: a measure.GirthRings."""
    ptr_, a, b, f = rings.tables()
    pt_ring, vt_ptr, vt_pt, vt_w, n_vt = rings.transposed()
    B, rows, P = v.shape[0], v.shape[1], ptr_.numel() - 1
    out = torch.empty((B, rows, 3), dtype=torch.float32, device=v.device)
    check(_lib.load().sh_measure_girth_bwd(ptr(v), v.stride(0) if B > 1 else rows * 3, ptr(ptr_), ptr(a), ptr(b), ptr(f), ptr(pt_ring),
                                           ptr(vt_ptr), ptr(vt_pt), ptr(vt_w), n_vt, ptr(g_girth), B, P, rows, ptr(out), stream_ptr()),
          "sh_measure_girth_bwd")
    return out


def bone_length_bwd(kps, bones, g_len):
    """Gradient of bone_length w.r.t. kps: -> [B, K, 3].  bones: a measure.Bones."""
    jt_ptr, jt_bone, jt_w, n_jt = bones.transposed()
    B, K, P = kps.shape[0], kps.shape[1], bones.n_bones
    out = torch.empty((B, K, 3), dtype=torch.float32, device=kps.device)
    check(_lib.load().sh_bone_length_bwd(ptr(kps), ptr(bones.table), ptr(jt_ptr), ptr(jt_bone), ptr(jt_w), n_jt, ptr(g_len), B, K, P,
                                         ptr(out), stream_ptr()), "sh_bone_length_bwd")
    return out


def joint_regress_bwd(g_kps, J, rows):
    """g_x = J^T g_kps for the first N rows, 0 for the rows behind them: g_kps contiguous [B, K, 3], J [K, N] -> [B, rows, 3]."""
    K, N = J.shape
    B = g_kps.shape[0]
    out = torch.empty((B, rows, 3), dtype=torch.float32, device=g_kps.device)
    check(_lib.load().sh_joint_regress_bwd(ptr(g_kps), ptr(J), B, N, K, rows, ptr(out), stream_ptr()), "sh_joint_regress_bwd")
    return out


def _points(t, what):
    """[B, rows, 3] fp32 HIP points with packed rows (the batch stride is free) -> (B, rows, batch stride in elements)."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.shape[2] == 3
            and (t.shape[1] == 0 or (t.stride(2) == 1 and t.stride(1) == 3))):
        raise RuntimeError("semantichuman_amd.%s needs fp32 HIP points [B, rows, 3] (got %s %s %s); there is no CPU path"
                           % (what, getattr(t, "device", None), getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
    B, rows = t.shape[0], t.shape[1]
    if B > 1 and t.stride(0) < 3 * rows:
        raise RuntimeError("semantichuman_amd.%s: bodies overlap in memory (batch stride %d < %d)" % (what, t.stride(0), 3 * rows))
    return B, rows, (t.stride(0) if B > 1 else rows * 3)


def _mask_arg(mask, B, rows, device):
    """None | bool/uint8 [rows] | [B, rows] -> (uint8 tensor or None, batch stride)."""
    if mask is None:
        return None, 0
    m = torch.as_tensor(mask, device=device)
    m = (m != 0).to(torch.uint8).contiguous()
    if m.dim() == 1 and m.shape[0] == rows:
        return m, 0
    if m.dim() == 2 and tuple(m.shape) == (B, rows):
        return m, rows
    raise ValueError("mask must be [%d] or [%d, %d], got %s" % (rows, B, rows, tuple(m.shape)))


def _count_arg(cnt, B, device):
    if cnt is None:
        return None
    c = torch.as_tensor(cnt, device=device).to(torch.int32).contiguous()
    if tuple(c.shape) != (B,):
        raise ValueError("per-body counts must be [%d], got %s" % (B, tuple(c.shape)))
    return c


def _face_table_arg(faces, who, what="face table"):
    """The model's triangles as the kernels take them, a contiguous int32 HIP tensor [nF, 3], checked -> nF."""
    if not (torch.is_tensor(faces) and faces.is_cuda and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3
            and faces.is_contiguous()):
        raise RuntimeError("semantichuman_amd.%s needs a contiguous int32 HIP %s [nF, 3] (scan.FaceTable makes one)" % (who, what))
    return faces.shape[0]


def nearest_points(q, t, q_count=None, t_count=None, t_mask=None, nq=None, nt=None, chunks=0, out=None, gate=None):
    """sh_nearest_points: q [B, *, 3] (the first nq rows are queries), t [B, *, 3] (the first nt rows are targets) ->
    (idx int32 [B, nq], d2 fp32 [B, nq]).  chunks: 0 = the library's split of the target range, k = that many ranges.
    gate: None, or (qn [B, >= nq, 3], tn [B, >= nt, 3], cos_min) - then sh_nearest_points_gated: only targets whose normal's fp32
    dot product with the query's reaches cos_min are candidates."""
    B, q_rows, q_sb = _points(q, "nearest_points")
    Bt, t_rows, t_sb = _points(t, "nearest_points")
    if Bt != B:
        raise ValueError("nearest_points: %d query bodies, %d target bodies" % (B, Bt))
    nq = q_rows if nq is None else int(nq)
    nt = t_rows if nt is None else int(nt)
    if not (0 <= nq <= q_rows and 0 <= nt <= t_rows):
        raise ValueError("nearest_points: nq / nt exceed the tensors' rows")
    q_count, t_count = _count_arg(q_count, B, q.device), _count_arg(t_count, B, q.device)
    mask, mask_sb = _mask_arg(t_mask, B, nt, q.device)
    lib = _lib.load()
    idx, d2 = out if out is not None else (torch.empty((B, nq), dtype=torch.int32, device=q.device),
                                          torch.empty((B, nq), dtype=torch.float32, device=q.device))
    nbytes = lib.sh_nearest_points_workspace(B, nq, nt, chunks)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device) if nbytes else None
    if gate is not None:
        qn, tn, cos_min = gate
        (Bq, qn_rows, qn_sb), (Bn, tn_rows, tn_sb) = _points(qn, "nearest_points (query normals)"), _points(tn, "nearest_points (target normals)")
        if Bq != B or Bn != B or qn_rows < nq or tn_rows < nt:
            raise ValueError("nearest_points: normals must be [%d, >= %d, 3] and [%d, >= %d, 3], got %s and %s"
                             % (B, nq, B, nt, tuple(qn.shape), tuple(tn.shape)))
        check(lib.sh_nearest_points_gated(ptr(q), q_sb, nq, ptr(q_count), ptr(qn), qn_sb, ptr(t), t_sb, nt, ptr(t_count), ptr(tn), tn_sb, ptr(mask),
                                          mask_sb, float(cos_min), B, chunks, ptr(idx), ptr(d2), ptr(ws), nbytes, stream_ptr()),
              "sh_nearest_points_gated")
        return idx, d2
    check(lib.sh_nearest_points(ptr(q), q_sb, nq, ptr(q_count), ptr(t), t_sb, nt, ptr(t_count), ptr(mask), mask_sb, B, chunks, ptr(idx),
                                ptr(d2), ptr(ws), nbytes, stream_ptr()), "sh_nearest_points")
    return idx, d2


def vertex_normals(x, faces, vf_ptr, vf_idx, n, out=None):
    """sh_vertex_normals: x [B, *, 3] of which the first n rows are vertices, faces int32 HIP [nF, 3] with its incidence (vf_ptr
    int32 [n + 1], vf_idx int32 [3 nF]; scan.FaceTable builds all three) -> unit normals, contiguous fp32 [B, n, 3]."""
    B, rows, x_sb = _points(x, "vertex_normals")
    n = int(n)
    if not 0 <= n <= rows:
        raise ValueError("vertex_normals: n = %d exceeds the model's %d rows" % (n, rows))
    nF = _face_table_arg(faces, "vertex_normals", "table faces")
    for t, shape, what in ((vf_ptr, (n + 1,), "vf_ptr [n + 1]"), (vf_idx, (3 * nF,), "vf_idx [3 nF]")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == shape):
            raise RuntimeError("semantichuman_amd.vertex_normals needs a contiguous int32 HIP table %s (scan.FaceTable makes one)" % what)
    nrm = out if out is not None else torch.empty((B, n, 3), dtype=torch.float32, device=x.device)
    check(_lib.load().sh_vertex_normals(ptr(x), x_sb, n, ptr(faces), nF, ptr(vf_ptr), ptr(vf_idx), B, ptr(nrm), stream_ptr()),
          "sh_vertex_normals")
    return nrm


CLOUD_K_MIN, CLOUD_K_MAX = 3, 64   # SH_CLOUD_K_MIN, SH_CLOUD_K_MAX


def cloud_normals(s, count=None, k=16, view=None, out=None):
    """sh_cloud_normals: s [B, M, 3] clouds, count [B] live rows per body (None = all), k neighbours (the point itself counts),
    view: None, fp32 HIP [B, 3] (one viewpoint per body) or [B, M, 3] (one per point) -> (nrm fp32 [B, M, 3], var fp32 [B, M],
    r2 fp32 [B, M], cnt int32 [B, M]), all contiguous; rows beyond a body's count are zero in all four."""
    B, M, s_sb = _points(s, "cloud_normals")
    k = int(k)
    if not CLOUD_K_MIN <= k <= CLOUD_K_MAX:
        raise ValueError("cloud_normals: k = %d outside [%d, %d]" % (k, CLOUD_K_MIN, CLOUD_K_MAX))
    count = _count_arg(count, B, s.device)
    view_sb = view_ps = 0
    if view is not None:
        if not (torch.is_tensor(view) and view.is_cuda and view.dtype == torch.float32 and view.is_contiguous()
                and tuple(view.shape) in ((B, 3), (B, M, 3))):
            raise ValueError("cloud_normals: view must be a contiguous fp32 HIP tensor [%d, 3] or [%d, %d, 3], got %s"
                             % (B, B, M, tuple(getattr(view, "shape", ()))))
        view_sb, view_ps = (3, 0) if view.dim() == 2 else (3 * M, 3)
    nrm, var, r2, cnt = out if out is not None else (torch.empty((B, M, 3), dtype=torch.float32, device=s.device),
                                                     torch.empty((B, M), dtype=torch.float32, device=s.device),
                                                     torch.empty((B, M), dtype=torch.float32, device=s.device),
                                                     torch.empty((B, M), dtype=torch.int32, device=s.device))
    check(_lib.load().sh_cloud_normals(ptr(s), s_sb, M, ptr(count), B, k, ptr(view), view_sb, view_ps, ptr(nrm), ptr(var), ptr(r2), ptr(cnt),
                                       None, 0, stream_ptr()), "sh_cloud_normals")
    return nrm, var, r2, cnt


MAX_VIEWS = 32                                                  # SH_VISIBILITY_MAX_VIEWS, SH_DEPTH_MAX_VIEWS


def _visibility(who, rig, x, faces, n, view, v_mask, tn, cos_g, chunks, out, seen=False):
    """`vertex_visibility` and `vertex_visibility_views` behind one set of checks.  rig False: view must be [B, 3], sh_vertex_visibility
    is called; rig True: view must be [B, V, 3], sh_vertex_visibility_views is called and can return the per-view bits.  who: the
    public name, for the messages only."""
    B, rows, x_sb = _points(x, who)
    n = int(n)
    if not 0 <= n <= rows:
        raise ValueError("%s: n = %d exceeds the model's %d rows" % (who, n, rows))
    nF = _face_table_arg(faces, who)
    if not (torch.is_tensor(view) and view.is_cuda and view.dtype == torch.float32 and view.is_contiguous() and view.dim() == (3 if rig else 2)
            and view.shape[0] == B and view.shape[-1] == 3):
        raise ValueError("%s: view must be a contiguous fp32 HIP tensor [%d, %s3], got %s" % (who, B, "V, " if rig else "", tuple(getattr(view, "shape", ()))))
    V = view.shape[1] if rig else 0
    if rig and not 1 <= V <= MAX_VIEWS:
        raise ValueError("%s: V = %d views, must lie in [1, %d]" % (who, V, MAX_VIEWS))
    if tn is not None and not (torch.is_tensor(tn) and tn.is_cuda and tn.dtype == torch.float32 and tn.is_contiguous()
                               and tuple(tn.shape) == (B, n, 3)):
        raise ValueError("%s: tn must be a contiguous fp32 HIP tensor [%d, %d, 3]" % (who, B, n))
    mask, mask_sb = _mask_arg(v_mask, B, n, x.device)
    chunks = int(chunks)
    if chunks < 0:
        raise ValueError("%s: chunks must be >= 0" % who)
    lib = _lib.load()
    vis = out if out is not None else torch.empty((B, n), dtype=torch.uint8, device=x.device)
    if not (torch.is_tensor(vis) and vis.device == x.device and vis.dtype == torch.uint8 and vis.is_contiguous() and tuple(vis.shape) == (B, n)):
        raise ValueError("%s: out must be a contiguous uint8 tensor [%d, %d] on the device of x" % (who, B, n))
    nbytes = lib.sh_vertex_visibility_views_workspace(B, n, nF, V, chunks) if rig else lib.sh_vertex_visibility_workspace(B, n, nF, chunks)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    head, tail = (ptr(x), x_sb, n, ptr(faces), nF, ptr(tn), ptr(view)), (float(cos_g), ptr(mask), mask_sb, B, chunks, ptr(ws), nbytes, ptr(vis))
    if not rig:
        check(lib.sh_vertex_visibility(*head, *tail, stream_ptr()), "sh_vertex_visibility")
        return vis
    bits = torch.empty((B, n), dtype=torch.int32, device=x.device) if seen else None
    check(lib.sh_vertex_visibility_views(*head, V, *tail, ptr(bits), stream_ptr()), "sh_vertex_visibility_views")
    return (vis, bits) if seen else vis


def vertex_visibility(x, faces, n, view, v_mask=None, tn=None, cos_g=0.0, chunks=0, out=None):
    """sh_vertex_visibility: x [B, *, 3] of which the first n rows are vertices, faces int32 HIP [nF, 3], view fp32 HIP [B, 3]
    (a NaN row: no viewpoint, every active vertex visible) -> uint8 [B, n], 1 = the vertex is active, not occluded by any face
    that does not name it and - with tn, contiguous fp32 [B, n, 3] vertex normals - faces the sensor to within cos_g.  v_mask
    [n] or [B, n].  chunks: 0 = the library's split of the face range, k = that many ranges; every split gives the same bits."""
    return _visibility("vertex_visibility", False, x, faces, n, view, v_mask, tn, cos_g, chunks, out)


def vertex_visibility_views(x, faces, n, view, v_mask=None, tn=None, cos_g=0.0, chunks=0, out=None, seen=False):
    """sh_vertex_visibility_views: `vertex_visibility` for a rig, view fp32 HIP [B, V, 3] with 1 <= V <= 32 (a NaN row: an absent
    camera; all rows NaN: a full scan) -> uint8 [B, n], 1 = some view sees the vertex; with seen=True -> (that, uint32 [B, n]
    carried as int32: bit v = view v alone sees it).  Every other argument as there."""
    return _visibility("vertex_visibility_views", True, x, faces, n, view, v_mask, tn, cos_g, chunks, out, seen)


DEPTH_DTYPES ={torch.float32: 0, torch.int16: 1}               # enum sh_depth_dtype: 16-bit words travel as int16 and are read unsigned


def _depth_args(who, rig, depth, intr, ext, mask, depth_scale, z_near, z_far, max_step, drop_isolated, stride):
    """The inputs the depth entry points share, checked -> (B, V, H, W, their C arguments up to `stride`).  rig True: a rig's depth
    [B, V, H, W] with ext [B, V, 12]; rig False: one camera's [B, H, W] - then V = 0 and ext is neither read nor among the arguments.
    who: the public name, for the messages only."""
    if not (torch.is_tensor(depth) and depth.is_cuda and depth.dtype in DEPTH_DTYPES and depth.dim() == (4 if rig else 3) and depth.is_contiguous()):
        raise RuntimeError("semantichuman_amd.%s needs a contiguous fp32 or 16-bit HIP depth image [B, %sH, W] (got %s %s %s); there is no CPU path"
                           % (who, "V, " if rig else "", getattr(depth, "device", None), getattr(depth, "dtype", type(depth)),
                              tuple(getattr(depth, "shape", ()))))
    lead, (H, W) = tuple(depth.shape[:-2]), depth.shape[-2:]
    B, V = lead[0], lead[1] if rig else 0
    if rig and not 1 <= V <= MAX_VIEWS:
        raise ValueError("%s: V = %d views, must lie in [1, %d]" % (who, V, MAX_VIEWS))
    for t, shape, what in ((intr, lead + (4,), "intr"), (ext, lead + (12,), "ext"))[:1 + rig]:
        if not (torch.is_tensor(t) and t.device == depth.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
            if not rig:
                raise ValueError("%s: intr must be a contiguous fp32 tensor [%d, 4] = (fx, fy, cx, cy) on the depth's device" % (who, B))
            raise ValueError("%s: %s %s = %s must be a contiguous fp32 tensor on the depth's device"
                             % (who, what, list(shape), "(fx, fy, cx, cy)" if t is intr else "(R row-major, t)"))
    if mask is not None and not (torch.is_tensor(mask) and mask.device == depth.device and mask.dtype == torch.uint8 and mask.is_contiguous()
                                 and mask.shape == depth.shape):
        raise ValueError("%s: mask must be a contiguous uint8 tensor %s on the depth's device" % (who, tuple(depth.shape)))
    stride = int(stride)
    if stride < 1:
        raise ValueError("%s: stride = %d, must be at least 1" % (who, stride))
    return B, V, H, W, ((ptr(depth), DEPTH_DTYPES[depth.dtype], float(depth_scale), ptr(intr), ptr(mask)) + ((ptr(ext), B, V) if rig else (B,))
                        + (H, W, float(z_near), float(z_far), float(max_step), int(bool(drop_isolated)), stride))


def _rays_arg(who, rays, B, V, H, W, device):
    """rays: None, or the calibration of "Camera rays" as (table fp32 [..., H, W, 2], dist fp32 [..., 8], limit fp32 [...]) with the
    leading shape [1] or [B] for one camera per body (V = 0), [V] or [B, V] for a rig: without the batch axis ONE table per
    camera serves every body -> (table, dist, limit, rays_stride), checked; rays_stride 0: shared."""
    if rays is None:
        return None
    table, dist, limit = rays
    per = max(V, 1)
    shared, own = ((V,) if V else (1,)), ((B, V) if V else (B,))
    lead = tuple(limit.shape) if torch.is_tensor(limit) else None
    if lead not in (shared, own) or not (_dense(table, device, torch.float32, lead + (H, W, 2)) and _dense(dist, device, torch.float32, lead + (8,))
                                         and _dense(limit, device, torch.float32, lead)):
        raise ValueError("%s: rays must be contiguous fp32 tensors (table %s, dist %s, limit %s) on the images' device, or the same with a leading "
                         "batch axis of %d" % (who, list(shared + (H, W, 2)), list(shared + (8,)), list(shared), B))
    return table, dist, limit, (0 if lead == shared and lead != own else per)


def camera_rays(intr, dist, H, W):
    """sh_camera_rays: intr fp32 [C, 4], dist fp32 [C, 8] on the GPU -> (rays fp32 [C, H, W, 2]: the pixel -> ray table, (NaN, NaN)
    where the inverse did not converge; limit fp32 [C]: the fold-back guard of the forward model; complete int32 [C]).  Two
    launches, nothing synchronised."""
    who = "camera_rays"
    if not (torch.is_tensor(intr) and intr.is_cuda and intr.dtype == torch.float32 and intr.dim() == 2 and intr.shape[1] == 4 and intr.is_contiguous()):
        raise ValueError("%s: intr must be a contiguous fp32 HIP tensor [C, 4]" % who)
    C, H, W = intr.shape[0], int(H), int(W)
    if not _dense(dist, intr.device, torch.float32, (C, 8)):
        raise ValueError("%s: dist must be a contiguous fp32 tensor [%d, 8] on the device of intr" % (who, C))
    if H < 0 or W < 0:
        raise ValueError("%s: negative image size (%d, %d)" % (who, H, W))
    rays = torch.empty((C, H, W, 2), dtype=torch.float32, device=intr.device)
    limit = torch.zeros((C,), dtype=torch.float32, device=intr.device)
    complete = torch.ones((C,), dtype=torch.int32, device=intr.device)
    check(_lib.load().sh_camera_rays(ptr(intr), ptr(dist), C, H, W, ptr(rays), ptr(limit), ptr(complete), stream_ptr()), "sh_" + who)
    return rays, limit, complete


def _depth_workspace(lib, B, V, H, W):
    """Bytes of the tile rows the count pass leaves for the points pass; V = 0: one camera."""
    return lib.sh_depth_views_workspace(B, V, H, W) if V else lib.sh_depth_workspace(B, H, W)


def _depth_entry(lib, rig, rays, what):
    """The entry point of the pass `what` ("count" / "points"): the rig's or one camera's, the "Camera rays" form with a table."""
    return getattr(lib, "sh_depth%s%s_%s" % ("_views" if rig else "", "_rays" if rays else "", what))


def _depth_count(who, rig, depth, *args, rays=None):
    """`depth_count` and `depth_views_count` (rig): args as `_depth_args` takes them after depth; rays as `_rays_arg` takes it."""
    B, V, H, W, cargs = _depth_args(who, rig, depth, *args)
    rays = _rays_arg(who, rays, B, V, H, W, depth.device)
    if rays:
        cargs += (ptr(rays[0]), rays[3])
    lib = _lib.load()
    counts = torch.empty((B,), dtype=torch.int32, device=depth.device)
    nbytes = _depth_workspace(lib, B, V, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=depth.device)
    check(_depth_entry(lib, rig, rays, "count")(*cargs, ptr(counts), ptr(ws), nbytes, stream_ptr()), "sh_" + who)
    return counts, ws


def _depth_points(who, rig, counts, workspace, M, max_count, depth, *args, rays=None):
    """`depth_points` and `depth_views_points` (rig): args as `_depth_args` takes them after depth; a rig's view and view_first are
    appended to the outputs; rays as `_rays_arg` takes it."""
    B, V, H, W, cargs = _depth_args(who, rig, depth, *args)
    rays = _rays_arg(who, rays, B, V, H, W, depth.device)
    if rays:
        cargs += (ptr(rays[0]), rays[3])
    M, max_count = int(M), int(max_count)
    counted = "depth_views_count" if rig else "depth_count"
    if not (torch.is_tensor(counts) and counts.device == depth.device and counts.dtype == torch.int32 and counts.is_contiguous()
            and tuple(counts.shape) == (B,)):
        raise ValueError("%s: counts must be the int32 tensor [%d] of %s" % (who, B, counted))
    lib = _lib.load()
    nbytes = _depth_workspace(lib, B, V, H, W)
    if not (torch.is_tensor(workspace) and workspace.device == depth.device and workspace.dtype == torch.uint8 and workspace.is_contiguous()
            and workspace.numel() >= nbytes):
        raise ValueError("%s: workspace must be the one %s returned for %s (%d bytes)"
                         % (who, counted, "these images" if rig else "this image", nbytes))
    points = torch.empty((B, max(M, 0), 3), dtype=torch.float32, device=depth.device)
    outs = (points, torch.empty_like(points), torch.empty((B, max(M, 0)), dtype=torch.int32, device=depth.device))
    if rig:
        outs += (torch.empty((B, max(M, 0)), dtype=torch.uint8, device=depth.device), torch.empty((B, V + 1), dtype=torch.int32, device=depth.device))
    check(_depth_entry(lib, rig, rays, "points")(*cargs, ptr(counts), max_count, M, ptr(workspace), workspace.numel(), *[ptr(t) for t in outs],
                                                 stream_ptr()), "sh_" + who)
    return outs


def depth_count(depth, intr, mask=None, depth_scale=1.0, z_near=-math.inf, z_far=math.inf, max_step=math.inf, drop_isolated=False, stride=1, rays=None):
    """sh_depth_count: depth [B, H, W] fp32 or 16-bit words on the device, intr fp32 [B, 4] = (fx, fy, cx, cy), mask uint8
    [B, H, W] or None -> (counts int32 [B], the kept pixels per body; the workspace sh_depth_points reads, the first row of every
    16 x 16 tile).  Nothing is synchronised.  rays: None, or the calibration of "Camera rays" (`_rays_arg`): sh_depth_rays_count."""
    return _depth_count("depth_count", False, depth, intr, None, mask, depth_scale, z_near, z_far, max_step, drop_isolated, stride, rays=rays)


def depth_points(depth, intr, counts, workspace, M, max_count, mask=None, depth_scale=1.0, z_near=-math.inf, z_far=math.inf, max_step=math.inf,
                 drop_isolated=False, stride=1, rays=None):
    """sh_depth_points: the inputs and options of the `depth_count` call that made (counts, workspace), a width M and the largest
    count as the caller read it (M >= max_count) -> (points fp32 [B, M, 3] in the camera's frame, normals fp32 [B, M, 3] - a
    zero row: unknown -, pixel int32 [B, M] = v * W + u), rows in tile / Z-order; beyond a body's count zeros, zeros and -1."""
    return _depth_points("depth_points", False, counts, workspace, M, max_count, depth, intr, None, mask, depth_scale, z_near, z_far, max_step,
                         drop_isolated, stride, rays=rays)


def depth_views_count(depth, intr, ext, mask=None, depth_scale=1.0, z_near=-math.inf, z_far=math.inf, max_step=math.inf, drop_isolated=False,
                      stride=1, rays=None):
    """sh_depth_views_count: depth [B, V, H, W] fp32 or 16-bit words on the device, intr fp32 [B, V, 4], ext fp32 [B, V, 12] (camera ->
    rig, R row-major then t; a NaN row: the view is absent), mask uint8 [B, V, H, W] or None -> (counts int32 [B], the kept pixels
    per body over its views; the workspace sh_depth_views_points reads).  Nothing is synchronised."""
    return _depth_count("depth_views_count", True, depth, intr, ext, mask, depth_scale, z_near, z_far, max_step, drop_isolated, stride, rays=rays)


def depth_views_points(depth, intr, ext, counts, workspace, M, max_count, mask=None, depth_scale=1.0, z_near=-math.inf, z_far=math.inf,
                       max_step=math.inf, drop_isolated=False, stride=1, rays=None):
    """sh_depth_views_points: the inputs and options of the `depth_views_count` call that made (counts, workspace), a width M and the
    largest count as the caller read it (M >= max_count) -> (points fp32 [B, M, 3] in the rig's frame, normals fp32 [B, M, 3],
    pixel int32 [B, M] = v * W + u in the row's view, view uint8 [B, M], view_first int32 [B, V + 1]); rows view-major, tile /
    Z-order inside a view; beyond a body's count zeros, zeros, -1 and 255."""
    return _depth_points("depth_views_points", True, counts, workspace, M, max_count, depth, intr, ext, mask, depth_scale, z_near, z_far, max_step,
                         drop_isolated, stride, rays=rays)


def _rig_rows(who, B, M, device, **planes):
    """The packed planes of a rig batch, checked: name=(tensor, dtype, trailing shape) -> nothing; ValueError for any that is not a
    contiguous tensor [B, M, ...] of that dtype on `device`."""
    for name, (t, dtype, tail) in planes.items():
        if not (torch.is_tensor(t) and t.device == device and t.dtype in (dtype if isinstance(dtype, tuple) else (dtype,)) and t.is_contiguous()
                and tuple(t.shape) == (B, M) + tail):
            raise ValueError("%s: %s must be a contiguous %s tensor %s on the device of the rest, got %s %s"
                             % (who, name, dtype, [B, M] + list(tail), getattr(t, "dtype", type(t).__name__), tuple(getattr(t, "shape", ()))))


_SEEN = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())


def depth_views_overlap(depth, intr, ext, points, normals, view, counts, tol, mask=None, depth_scale=1.0, z_near=-math.inf, z_far=math.inf, rays=None):
    """sh_depth_views_overlap: the images, calibration and range of the `depth_views_count` / `depth_views_points` calls that made the
    packed rows (points, normals fp32 [B, M, 3], view uint8 [B, M], counts int32 [B]) and a depth tolerance tol >= 0 -> (seen int32
    [B, M] read as unsigned: bit c set where camera c measures the row's surface point within tol, the row's own bit always; keep
    uint8 [B, M]: 0 where an observing camera is better placed - larger cos / d^2 under the row's normal, the lower index on a
    tie); zeros in the padding.  One launch, nothing synchronised.  rays: None, or the calibration of "Camera rays"
    (`_rays_arg`): sh_depth_views_rays_overlap, the projection under the lens model."""
    who = "depth_views_overlap"
    B, V, H, W, cargs = _depth_args(who, True, depth, intr, ext, mask, depth_scale, z_near, z_far, math.inf, False, 1)
    rays = _rays_arg(who, rays, B, V, H, W, depth.device)
    tol = float(tol)
    if not tol >= 0:
        raise ValueError("%s: tol must be >= 0, got %r" % (who, tol))
    M = points.shape[1] if torch.is_tensor(points) and points.dim() == 3 else -1
    _rig_rows(who, B, M, depth.device, points=(points, torch.float32, (3,)), normals=(normals, torch.float32, (3,)), view=(view, torch.uint8, ()))
    if not (torch.is_tensor(counts) and counts.device == depth.device and counts.dtype == torch.int32 and counts.is_contiguous()
            and tuple(counts.shape) == (B,)):
        raise ValueError("%s: counts must be the int32 tensor [%d] of the packed rows" % (who, B))
    seen = torch.empty((B, M), dtype=torch.int32, device=depth.device)
    keep = torch.empty((B, M), dtype=torch.uint8, device=depth.device)
    lib, cal = _lib.load(), ()
    if rays:
        cal = (ptr(rays[1]), ptr(rays[2]), rays[3])
    check((lib.sh_depth_views_rays_overlap if rays else lib.sh_depth_views_overlap)(*cargs[:12], *cal, ptr(points), ptr(normals), ptr(view), ptr(counts),
                                                                                    M, tol, ptr(seen), ptr(keep), stream_ptr()), "sh_" + who)
    return seen, keep


def scan_compact(points, normals, pixel, view, keep, counts, V, M_out, max_kept, seen=None):
    """sh_scan_compact: a rig batch's planes (points, normals fp32 [B, M, 3], pixel int32, view uint8, seen int32 or None, all
    [B, M]; counts int32 [B]), a keep plane uint8 [B, M], a width M_out and the largest kept count as the caller read it
    (M_out >= max_kept) -> (points, normals, pixel, view, seen or None, counts int32 [B], view_first int32 [B, V + 1]) at width
    M_out: the kept live rows in their old order, then zeros, zeros, -1, 255 and 0.  Three launches, nothing synchronised."""
    who = "scan_compact"
    if not (torch.is_tensor(points) and points.is_cuda and points.dim() == 3):
        raise RuntimeError("semantichuman_amd.%s needs fp32 HIP points [B, M, 3] (got %s %s); there is no CPU path"
                           % (who, getattr(points, "device", None), tuple(getattr(points, "shape", ()))))
    B, M, _ = points.shape
    V, M_out, max_kept = int(V), int(M_out), int(max_kept)
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError("%s: V = %d views, must lie in [1, %d]" % (who, V, MAX_VIEWS))
    planes = dict(points=(points, torch.float32, (3,)), normals=(normals, torch.float32, (3,)), pixel=(pixel, torch.int32, ()),
                  view=(view, torch.uint8, ()), keep=(keep, torch.uint8, ()))
    if seen is not None:
        planes["seen"] = (seen, _SEEN, ())
    _rig_rows(who, B, M, points.device, **planes)
    if not (torch.is_tensor(counts) and counts.device == points.device and counts.dtype == torch.int32 and counts.is_contiguous()
            and tuple(counts.shape) == (B,)):
        raise ValueError("%s: counts must be an int32 tensor [%d] on the points' device" % (who, B))
    lib = _lib.load()
    dev, width = points.device, max(M_out, 0)
    outs = [torch.empty((B, width, 3), dtype=torch.float32, device=dev), torch.empty((B, width, 3), dtype=torch.float32, device=dev),
            torch.empty((B, width), dtype=torch.int32, device=dev), torch.empty((B, width), dtype=torch.uint8, device=dev),
            None if seen is None else torch.empty((B, width), dtype=seen.dtype, device=dev),
            torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, V + 1), dtype=torch.int32, device=dev)]
    nbytes = lib.sh_scan_compact_workspace(B, M)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib.sh_scan_compact(ptr(points), ptr(normals), ptr(pixel), ptr(view), ptr(seen), ptr(keep), ptr(counts), B, V, M, max_kept, M_out,
                              ptr(ws), nbytes, *[ptr(t) for t in outs], stream_ptr()), "sh_" + who)
    return tuple(outs)


def depth_field(depth, intr, mask=None, depth_scale=1.0, z_near=-math.inf, z_far=math.inf):
    """sh_depth_field: the image inputs of `depth_count` -> (cls uint8 [B, H, W]: 0 empty, 1 unknown, 2 surface; z fp32 [B, H, W],
    the surface depth; nearest int32 [B, H, W], the nearest pixel that is not empty as v * W + u, -1: the image has none).
    Nothing is synchronised."""
    B, _, H, W, args = _depth_args("depth_field", False, depth, intr, None, mask, depth_scale, z_near, z_far, math.inf, False, 1)
    lib = _lib.load()
    cls = torch.empty((B, H, W), dtype=torch.uint8, device=depth.device)
    z = torch.empty((B, H, W), dtype=torch.float32, device=depth.device)
    nearest = torch.empty((B, H, W), dtype=torch.int32, device=depth.device)
    nbytes = lib.sh_depth_field_workspace(B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=depth.device)
    check(lib.sh_depth_field(*args[:10], ptr(cls), ptr(z), ptr(nearest), ptr(ws), nbytes, stream_ptr()), "sh_depth_field")
    return cls, z, nearest


def _dense(t, device, dtype, shape):
    return torch.is_tensor(t) and t.device == device and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()


def _free_space_args(who, rig, x, n, cam, cls, z, nearest, intr, v_mask, mask_sb, margin, rays=None):
    """The arguments the free-space entry points share, checked -> (B, lead, rows, their C arguments up to `margin`).  rig True: a
    rig's field [B, V, H, W] with intr [B, V, 4] and cam [B, V, 12], lead = (B, V); rig False: one camera's [B, H, W] and [B, 4],
    lead = (B,) - then cam is neither read nor among the arguments.  who: the public name, for the messages only."""
    B, rows, x_sb = _points(x, who)
    n = int(n)
    if not 0 <= n <= rows:
        raise ValueError("%s: n = %d exceeds the model's %d rows" % (who, n, rows))
    if not (torch.is_tensor(cls) and cls.device == x.device and cls.dtype == torch.uint8 and cls.dim() == (4 if rig else 3) and cls.shape[0] == B
            and cls.is_contiguous()):
        raise ValueError("%s: cls must be a contiguous uint8 tensor [%d, %sH, W] on the device of x" % (who, B, "V, " if rig else ""))
    lead, (H, W) = tuple(cls.shape[:-2]), cls.shape[-2:]
    if rig and not 1 <= lead[1] <= MAX_VIEWS:
        raise ValueError("%s: V = %d views, must lie in [1, %d]" % (who, lead[1], MAX_VIEWS))
    planes = [(z, torch.float32, lead + (H, W), "z fp32"), (nearest, torch.int32, lead + (H, W), "nearest int32"),
              (intr, torch.float32, lead + (4,), "intr fp32")]
    if rig:
        planes.append((cam, torch.float32, lead + (12,), "cam fp32"))
    for t, dtype, shape, what in planes:
        if not _dense(t, x.device, dtype, shape):
            raise ValueError("%s: %s must be a contiguous tensor %s on the device of x" % (who, what, list(shape)))
    head, field, tail = (ptr(x), x_sb, rows, n), (ptr(cls), ptr(z), ptr(nearest), ptr(intr)), (H, W, ptr(v_mask), mask_sb, float(margin))
    if rays is not None:                                                # "Camera rays": one entry-point pair, cam NULL for one camera
        rays = _rays_arg(who, rays, B, lead[1] if rig else 0, H, W, x.device)
        return B, lead, rows, head + (ptr(cam if rig else None),) + field + (ptr(rays[0]), ptr(rays[1]), ptr(rays[2]), rays[3], lead[1] if rig else 1) + tail
    if rig:
        return B, lead, rows, head + (ptr(cam),) + field + (lead[1],) + tail
    return B, lead, rows, head + field + tail


def _free_space_entry(rig, rays, what):
    """-> (the public name for the messages, the entry point's): with a calibration the _views_rays_ pair serves both."""
    who = "free_space_views_" + what if rig else "free_space_" + what
    return who, "sh_free_space_views_rays_" + what if rays is not None else "sh_" + who


def _free_space_fwd(rig, x, n, cam, cls, z, nearest, intr, v_mask, mask_sb, margin, rays=None):
    """`free_space_fwd` and `free_space_views_fwd` (rig) behind one set of checks; the outputs carry the field's leading shape.
    rays: None, or the calibration of "Camera rays" (`_rays_arg`): sh_free_space_views_rays_fwd."""
    who, entry = _free_space_entry(rig, rays, "fwd")
    B, lead, rows, args = _free_space_args(who, rig, x, n, cam, cls, z, nearest, intr, v_mask, mask_sb, margin, rays)
    term = torch.empty(lead + (int(n),), dtype=torch.float32, device=x.device)
    kind = torch.empty(lead + (int(n),), dtype=torch.uint8, device=x.device)
    loss = torch.empty((B, 2), dtype=torch.float32, device=x.device)
    counts = torch.empty(lead + (4,), dtype=torch.int32, device=x.device)
    check(getattr(_lib.load(), entry)(*args, B, ptr(term), ptr(kind), ptr(loss), ptr(counts), stream_ptr()), entry)
    return term, kind, loss, counts


def _free_space_bwd(rig, x, n, cam, cls, z, nearest, intr, v_mask, mask_sb, margin, counts, gL, rays=None):
    """`free_space_bwd` and `free_space_views_bwd` (rig) behind one set of checks; rays as in `_free_space_fwd`."""
    who, entry = _free_space_entry(rig, rays, "bwd")
    B, lead, rows, args = _free_space_args(who, rig, x, n, cam, cls, z, nearest, intr, v_mask, mask_sb, margin, rays)
    if not _dense(gL, x.device, torch.float32, (B, 2)):
        raise ValueError("%s: gL must be a contiguous fp32 tensor [%d, 2] on the device of x" % (who, B))
    if rig and not _dense(counts, x.device, torch.int32, lead + (4,)):     # one camera's counts were never checked here
        raise ValueError("%s: counts must be the forward call's int32 tensor %s" % (who, list(lead + (4,))))
    g = torch.empty((B, rows, 3), dtype=torch.float32, device=x.device)
    check(getattr(_lib.load(), entry)(*args, ptr(counts), ptr(gL), B, ptr(g), stream_ptr()), entry)
    return g


def free_space_fwd(x, n, cls, z, nearest, intr, v_mask=None, mask_sb=0, margin=0.0):
    """sh_free_space_fwd: x [B, *, 3] camera-frame points of which the first n rows are vertices, a depth field (cls, z, nearest)
    and intr [B, 4] of the same B; v_mask uint8 [n] (mask_sb 0) or [B, n] (mask_sb n), as `_mask_arg` makes it -> (term fp32
    [B, n], kind uint8 [B, n], loss fp32 [B, 2] = (free space, silhouette), counts int32 [B, 4] = (active, kind 1, 2, 4))."""
    return _free_space_fwd(False, x, n, None, cls, z, nearest, intr, v_mask, mask_sb, margin)


def free_space_bwd(x, n, cls, z, nearest, intr, v_mask, mask_sb, margin, counts, gL):
    """sh_free_space_bwd: the forward call's arguments, its counts and gL fp32 [B, 2] -> g_x contiguous [B, rows, 3] (every element
    written)."""
    return _free_space_bwd(False, x, n, None, cls, z, nearest, intr, v_mask, mask_sb, margin, counts, gL)


def free_space_cameras(ext, pose=None):
    """sh_free_space_cameras: ext fp32 [B, V, 12] on the GPU (camera -> rig, R row-major then t: `scan.pack_extrinsics`' layout) and
    pose fp32 [B, 12] (`Pose.packed`: scan / rig frame -> model frame) or None, the identity -> cam fp32 [B, V, 12] = (M | c), model
    frame -> camera frame: M = R^T A^-1, c = -R^T (A^-1 t + t_v), fp64 inside, rounded once; NaN rows for an absent camera or a
    singular pose.  One launch."""
    who = "free_space_cameras"
    if not (torch.is_tensor(ext) and ext.is_cuda and ext.dtype == torch.float32 and ext.dim() == 3 and ext.shape[2] == 12 and ext.is_contiguous()):
        raise ValueError("%s: ext must be a contiguous fp32 HIP tensor [B, V, 12]" % who)
    B, V = ext.shape[:2]
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError("%s: V = %d views, must lie in [1, %d]" % (who, V, MAX_VIEWS))
    if pose is not None and not _dense(pose, ext.device, torch.float32, (B, 12)):
        raise ValueError("%s: pose must be a contiguous fp32 tensor [%d, 12] on the device of ext" % (who, B))
    cam = torch.empty((B, V, 12), dtype=torch.float32, device=ext.device)
    check(_lib.load().sh_free_space_cameras(ptr(pose), ptr(ext), B, V, ptr(cam), stream_ptr()), "sh_" + who)
    return cam


def free_space_views_fwd(x, n, cam, cls, z, nearest, intr, v_mask=None, mask_sb=0, margin=0.0):
    """sh_free_space_views_fwd: x [B, *, 3] model-frame points of which the first n rows are vertices, cam [B, V, 12]
    (`free_space_cameras`), a rig's depth field (cls, z, nearest [B, V, H, W]) and intr [B, V, 4]; v_mask as in `free_space_fwd`
    -> (term fp32 [B, V, n], kind uint8 [B, V, n], loss fp32 [B, 2] = (free space, silhouette) summed over the views, counts int32
    [B, V, 4] = (active, kind 1, 2, 4) per view)."""
    return _free_space_fwd(True, x, n, cam, cls, z, nearest, intr, v_mask, mask_sb, margin)


def free_space_views_bwd(x, n, cam, cls, z, nearest, intr, v_mask, mask_sb, margin, counts, gL):
    """sh_free_space_views_bwd: the forward call's arguments, its counts [B, V, 4] and gL fp32 [B, 2] -> g_x contiguous
    [B, rows, 3] in the frame of x (every element written)."""
    return _free_space_bwd(True, x, n, cam, cls, z, nearest, intr, v_mask, mask_sb, margin, counts, gL)


ROBUST_FORMS = {"geman-mcclure": 1, "huber": 2}                # enum sh_robust (0: none)


def _robust_entry(entry, robust):
    """How every wrapper with a `robust` argument picks its C entry point: None -> (entry, no extra arguments), the plain call,
    exactly as ever; (form id, scale2) -> (entry + "_robust", those two)."""
    return (entry, ()) if robust is None else (entry + "_robust", (int(robust[0]), float(robust[1])))


def chamfer_fwd(d2_sm, s_count, d2_ms, rows, n, v_mask, mask_sb, tau2, w_ms, out=None, robust=None):
    """sh_chamfer_fwd -> (loss [B], counts int32 [B, 2]).  robust: None, or (form id of ROBUST_FORMS, scale2) - then
    sh_chamfer_fwd_robust; so in every wrapper below that takes it."""
    B, M = d2_sm.shape
    loss, counts = out if out is not None else (torch.empty(B, dtype=torch.float32, device=d2_sm.device),
                                                torch.empty((B, 2), dtype=torch.int32, device=d2_sm.device))
    entry, extra = _robust_entry("sh_chamfer_fwd", robust)
    check(getattr(_lib.load(), entry)(ptr(d2_sm), M, ptr(s_count), ptr(d2_ms), rows, n, ptr(v_mask), mask_sb, tau2, w_ms, B, ptr(loss),
                                      ptr(counts), stream_ptr(), *extra), entry)
    return loss, counts


def _chamfer_bwd(entry, x, n, s, s_count, partner, idx_ms, d2_ms, v_mask, mask_sb, counts, tau2, w_ms, gL, out, robust=None):
    """Both gradient wrappers: C entry point `entry` -> g_x contiguous [B, rows, 3] (every element written).  partner: the C
    arguments of the scan -> model partner, (idx_sm, d2_sm) or (faces, nF, face, d2, uv)."""
    entry, extra = _robust_entry(entry, robust)
    who = entry[3:]
    B, rows, x_sb = _points(x, who)
    _, M, s_sb = _points(s, who)
    g = out if out is not None else torch.empty((B, rows, 3), dtype=torch.float32, device=x.device)
    check(getattr(_lib.load(), entry)(ptr(x), x_sb, rows, n, ptr(s), s_sb, M, ptr(s_count), *partner, ptr(idx_ms), ptr(d2_ms), ptr(v_mask), mask_sb,
                                      ptr(counts), tau2, w_ms, ptr(gL), B, ptr(g), stream_ptr(), *extra), entry)
    return g


def chamfer_bwd(x, n, s, s_count, idx_sm, d2_sm, idx_ms, d2_ms, v_mask, mask_sb, counts, tau2, w_ms, gL, out=None, robust=None):
    """sh_chamfer_bwd -> g_x contiguous [B, rows, 3] (every element written)."""
    return _chamfer_bwd("sh_chamfer_bwd", x, n, s, s_count, (ptr(idx_sm), ptr(d2_sm)), idx_ms, d2_ms, v_mask, mask_sb, counts, tau2, w_ms, gL, out,
                        robust)


def face_normals(x, faces, n, out=None):
    """sh_face_normals: x [B, *, 3] of which the first n rows are vertices, faces int32 HIP [nF, 3] -> unit face normals,
    contiguous fp32 [B, nF, 3] (zero for a face without area or with a corner outside [0, n))."""
    B, rows, x_sb = _points(x, "face_normals")
    n = int(n)
    if not 0 <= n <= rows:
        raise ValueError("face_normals: n = %d exceeds the model's %d rows" % (n, rows))
    nF = _face_table_arg(faces, "face_normals")
    nrm = out if out is not None else torch.empty((B, nF, 3), dtype=torch.float32, device=x.device)
    check(_lib.load().sh_face_normals(ptr(x), x_sb, n, ptr(faces), nF, B, ptr(nrm), stream_ptr()), "sh_face_normals")
    return nrm


def nearest_surface(q, x, faces, n, q_count=None, v_mask=None, bound=None, chunks=0, cull=True, out=None, stats=None, gate=None):
    """sh_nearest_surface: q [B, *, 3] scan points, x [B, *, 3] model points of which the first n are vertices, faces int32 HIP
    [nF, 3] (one table for the batch) -> (face int32 [B, nq], d2 fp32 [B, nq], uv fp32 [B, nq, 2]).  bound [B, nq]: an upper
    bound of each answer (the squared distance to the nearest vertex), None = none; cull=False runs every pair through the region
    test (the yardstick: same bits).  stats: None or a zeroed int64 HIP tensor [2] that receives (region tests run, points swept again without a bound).
    gate: None, or (qn [B, >= nq, 3], fn contiguous [B, nF, 3] from `face_normals`, cos_min) - then sh_nearest_surface_gated: only
    the faces whose normal's fp32 dot product with the point's reaches cos_min are candidates, and with bound=None the library
    bounds the culled sweep itself (the gated search over the face centres)."""
    B, nq, q_sb = _points(q, "nearest_surface")
    Bx, x_rows, x_sb = _points(x, "nearest_surface")
    if Bx != B:
        raise ValueError("nearest_surface: %d scan bodies, %d model bodies" % (B, Bx))
    n = int(n)
    if not 0 <= n <= x_rows:
        raise ValueError("nearest_surface: n = %d exceeds the model's %d rows" % (n, x_rows))
    nF = _face_table_arg(faces, "nearest_surface")
    q_count = _count_arg(q_count, B, q.device)
    mask, mask_sb = _mask_arg(v_mask, B, n, q.device)
    if bound is not None and not (bound.is_cuda and bound.dtype == torch.float32 and bound.is_contiguous() and tuple(bound.shape) == (B, nq)):
        raise RuntimeError("semantichuman_amd.nearest_surface: bound must be a contiguous fp32 HIP tensor [%d, %d]" % (B, nq))
    lib = _lib.load()
    face, d2, uv = out if out is not None else (torch.empty((B, nq), dtype=torch.int32, device=q.device),
                                                torch.empty((B, nq), dtype=torch.float32, device=q.device),
                                                torch.empty((B, nq, 2), dtype=torch.float32, device=q.device))
    if gate is not None:
        qn, fn, cos_min = gate
        Bq, qn_rows, qn_sb = _points(qn, "nearest_surface (scan normals)")
        if Bq != B or qn_rows < nq:
            raise ValueError("nearest_surface: scan normals must be [%d, >= %d, 3], got %s" % (B, nq, tuple(qn.shape)))
        if not (torch.is_tensor(fn) and fn.is_cuda and fn.dtype == torch.float32 and fn.is_contiguous() and tuple(fn.shape) == (B, nF, 3)):
            raise RuntimeError("semantichuman_amd.nearest_surface: face normals must be a contiguous fp32 HIP tensor [%d, %d, 3]" % (B, nF))
        nbytes = lib.sh_nearest_surface_gated_workspace(B, nq, nF, chunks)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device) if nbytes else None
        check(lib.sh_nearest_surface_gated(ptr(q), q_sb, nq, ptr(q_count), ptr(qn), qn_sb, ptr(x), x_sb, n, ptr(faces), nF, ptr(fn), ptr(mask),
                                           mask_sb, float(cos_min), ptr(bound), B, chunks, 1 if cull else 0, ptr(face), ptr(d2), ptr(uv),
                                           ptr(stats), ptr(ws), nbytes, stream_ptr()), "sh_nearest_surface_gated")
        return face, d2, uv
    nbytes = lib.sh_nearest_surface_workspace(B, nq, nF, chunks)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device) if nbytes else None
    check(lib.sh_nearest_surface(ptr(q), q_sb, nq, ptr(q_count), ptr(x), x_sb, n, ptr(faces), nF, ptr(mask), mask_sb, ptr(bound), B, chunks,
                                 1 if cull else 0, ptr(face), ptr(d2), ptr(uv), ptr(stats), ptr(ws), nbytes, stream_ptr()), "sh_nearest_surface")
    return face, d2, uv


def chamfer_surface_bwd(x, n, s, s_count, faces, face, d2, uv, idx_ms, d2_ms, v_mask, mask_sb, counts, tau2, w_ms, gL, out=None, robust=None):
    """sh_chamfer_surface_bwd -> g_x contiguous [B, rows, 3] (every element written)."""
    return _chamfer_bwd("sh_chamfer_surface_bwd", x, n, s, s_count, (ptr(faces), faces.shape[0], ptr(face), ptr(d2), ptr(uv)), idx_ms, d2_ms,
                        v_mask, mask_sb, counts, tau2, w_ms, gL, out, robust)


ALIGN_MODES = {"translation": 0, "rigid": 1, "similarity": 2}   # enum sh_align_mode
ALIGN_PARTIAL, ALIGN_MOMENTS = 19, 20                           # SH_ALIGN_PARTIAL, SH_ALIGN_MOMENTS


def _surface_partner(who, faces, face, uv, d2, B, M):
    """The scan -> model partner of a surface moments call, checked: the table `faces` (int32 HIP [nF, 3]) and what
    sh_nearest_surface recorded on it; returns the C arguments that take the place of (idx_sm, d2_sm)."""
    nF = _face_table_arg(faces, who)
    for t, dtype, shape, what in ((face, torch.int32, (B, M), "face"), (d2, torch.float32, (B, M), "d2"), (uv, torch.float32, (B, M, 2), "uv")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape):
            raise RuntimeError("semantichuman_amd.%s: %s must be a contiguous %s HIP tensor %s" % (who, what, dtype, list(shape)))
    return ptr(faces), nF, ptr(face), ptr(uv), ptr(d2)


def _align_moments(entry, per_range, s, s_count, x, n, v_mask, mask_sb, idx_sm, d2_sm, idx_ms, d2_ms, tau2, w_ms, out, normals=None, surface=None,
                   robust=None):
    """The four moments wrappers: C entry point `entry` -> the ranges' partial sums, fp64 [B, ranges, per_range].  normals: None, or
    (tn, needed) of a point-to-plane call; surface: None, or (faces, face, uv, d2), the partner instead of (idx_sm, d2_sm)."""
    entry, extra = _robust_entry(entry, robust)
    who = entry[3:]
    B, M, s_sb = _points(s, who)
    _, rows, x_sb = _points(x, who)
    tn = () if normals is None else (ptr(_plane_normals(normals[0], B, n, who, normals[1])),)
    partner = (ptr(idx_sm), ptr(d2_sm)) if surface is None else _surface_partner(who, *surface, B, M)
    lib = _lib.load()
    part = out if out is not None else torch.empty((B, lib.sh_align_ranges(M, n, w_ms), per_range), dtype=torch.float64, device=s.device)
    check(getattr(lib, entry)(ptr(s), s_sb, M, ptr(s_count), ptr(x), x_sb, rows, n, ptr(v_mask), mask_sb, *tn, *partner, ptr(idx_ms), ptr(d2_ms),
                              tau2, w_ms, B, ptr(part), part.numel() * 8, stream_ptr(), *extra), entry)
    return part


def align_moments(s, s_count, x, n, v_mask, mask_sb, idx_sm, d2_sm, idx_ms, d2_ms, tau2, w_ms, out=None, robust=None):
    """sh_align_moments -> the ranges' partial sums, fp64 [B, ranges, 19] (stage 1; sh_align_solve finishes them)."""
    return _align_moments("sh_align_moments", ALIGN_PARTIAL, s, s_count, x, n, v_mask, mask_sb, idx_sm, d2_sm, idx_ms, d2_ms, tau2, w_ms, out,
                          robust=robust)


def align_moments_surface(s, s_count, x, n, v_mask, mask_sb, faces, face, uv, d2, idx_ms, d2_ms, tau2, w_ms, out=None, robust=None):
    """sh_align_moments_surface -> the ranges' partial sums, fp64 [B, ranges, 19]: sh_align_moments with the scan -> model partner
    the foot point (face, uv) that sh_nearest_surface recorded on the table `faces` (int32 HIP [nF, 3]); d2 is the surface
    distance."""
    return _align_moments("sh_align_moments_surface", ALIGN_PARTIAL, s, s_count, x, n, v_mask, mask_sb, None, None, idx_ms, d2_ms, tau2, w_ms, out,
                          surface=(faces, face, uv, d2), robust=robust)


def align_solve(part, M, n, s_count, w_ms, mode, pose=None, scale=None, pose_out=None, scale_out=None, inc=None, mom=None):
    """sh_align_solve: partial sums -> moments (mom fp64 [B, 20], optional), the pose increment (inc fp32 [B, 13], optional) and
    the pose (pose fp32 [B, 12], scale [B]) composed with it into pose_out / scale_out (which may be pose / scale themselves)."""
    B = part.shape[0]
    check(_lib.load().sh_align_solve(ptr(part), M, n, ptr(s_count), w_ms, ALIGN_MODES[mode], B, ptr(pose), ptr(scale), ptr(pose_out), ptr(scale_out),
                                     ptr(inc), ptr(mom), stream_ptr()), "sh_align_solve")


ALIGN_PLANE_PARTIAL, ALIGN_PLANE_SYSTEM = 38, 37                # SH_ALIGN_PLANE_PARTIAL, SH_ALIGN_PLANE_SYSTEM


def _plane_normals(tn, B, n, what, needed):
    """The vertex normals a point-to-plane call takes: None (allowed only where none are read) or contiguous fp32 HIP [B, n, 3]."""
    if tn is None:
        if needed:
            raise RuntimeError("semantichuman_amd.%s needs the vertex normals tn [%d, %d, 3] (sh_vertex_normals)" % (what, B, n))
        return None
    if not (torch.is_tensor(tn) and tn.is_cuda and tn.dtype == torch.float32 and tn.is_contiguous() and tuple(tn.shape) == (B, n, 3)):
        raise RuntimeError("semantichuman_amd.%s: tn must be a contiguous fp32 HIP tensor [%d, %d, 3]" % (what, B, n))
    return tn


def align_plane_moments(s, s_count, x, n, v_mask, mask_sb, tn, idx_sm, d2_sm, idx_ms, d2_ms, tau2, w_ms, out=None, robust=None):
    """sh_align_plane_moments -> the ranges' partial sums of the point-to-plane step, fp64 [B, ranges, 38] (stage 1;
    sh_align_plane_solve finishes them).  tn: the vertex normals, contiguous fp32 [B, n, 3]."""
    return _align_moments("sh_align_plane_moments", ALIGN_PLANE_PARTIAL, s, s_count, x, n, v_mask, mask_sb, idx_sm, d2_sm, idx_ms, d2_ms, tau2, w_ms,
                          out, normals=(tn, True), robust=robust)


def align_plane_moments_surface(s, s_count, x, n, v_mask, mask_sb, tn, faces, face, uv, d2, idx_ms, d2_ms, tau2, w_ms, out=None, robust=None):
    """sh_align_plane_moments_surface -> fp64 [B, ranges, 38]: sh_align_plane_moments with the scan -> model partner the foot point
    (face, uv) that sh_nearest_surface recorded on the table `faces` and the normal that face's; tn (the model -> scan pairs'
    normals) may be None when w_ms == 0."""
    return _align_moments("sh_align_plane_moments_surface", ALIGN_PLANE_PARTIAL, s, s_count, x, n, v_mask, mask_sb, None, None, idx_ms, d2_ms, tau2,
                          w_ms, out, normals=(tn, w_ms > 0), surface=(faces, face, uv, d2), robust=robust)


def align_plane_solve(part, M, n, s_count, w_ms, mode, pose=None, scale=None, pose_out=None, scale_out=None, sys=None, solved=None):
    """sh_align_plane_solve: partial sums -> the joined system (sys fp64 [B, 37], optional), its Gauss-Newton increment composed
    with the pose (pose fp32 [B, 12], scale [B]) into pose_out / scale_out (which may be pose / scale themselves), and solved int32
    [B] (0: the system was singular and the pose passed through); returns solved."""
    B = part.shape[0]
    if pose_out is not None and solved is None:
        solved = torch.empty(B, dtype=torch.int32, device=part.device)
    check(_lib.load().sh_align_plane_solve(ptr(part), M, n, ptr(s_count), w_ms, ALIGN_MODES[mode], B, ptr(pose), ptr(scale), ptr(pose_out),
                                           ptr(scale_out), ptr(sys), ptr(solved), stream_ptr()), "sh_align_plane_solve")
    return solved


def transform_points(src, count, pose, out=None):
    """sh_transform_points: dst[b, j] = A_b src[b, j] + t_b for j < count[b], zero rows beyond; pose fp32 contiguous [B, 12]."""
    B, M, src_sb = _points(src, "transform_points")
    if not (pose.is_cuda and pose.dtype == torch.float32 and pose.is_contiguous() and tuple(pose.shape) == (B, 12)):
        raise RuntimeError("semantichuman_amd.transform_points needs a contiguous fp32 HIP pose [%d, 12]" % B)
    dst = out if out is not None else torch.empty((B, M, 3), dtype=torch.float32, device=src.device)
    check(_lib.load().sh_transform_points(ptr(src), src_sb, M, ptr(count), ptr(pose), B, ptr(dst), stream_ptr()), "sh_transform_points")
    return dst


NORM_FLAGS = {"zeromean": 1, "zeroroot": 2, "onelength": 4, "small": 8, "gass": 16, "normal": 32}


def dataset_normalize(raw, flags, dummy_rows=1, j_root=None, mean=None, std=None, center=None, scale=None):
    """raw [n, N, 3] fp32 HIP tensor -> normalised, dummy-padded [n, N + dummy_rows, 3]."""
    if not (raw.is_cuda and raw.dtype == torch.float32 and raw.dim() == 3 and raw.shape[2] == 3 and raw.is_contiguous()):
        raise RuntimeError("semantichuman_amd.dataset_normalize needs a contiguous fp32 HIP tensor [n, N, 3]; there is no CPU path")
    n, N = raw.shape[0], raw.shape[1]
    for t, shape in ((j_root, (N,)), (mean, (N, 3)), (std, (N, 3)), (center, (n, 3)), (scale, (n, 3))):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
            raise RuntimeError("dataset_normalize: table must be a contiguous fp32 HIP tensor of shape %s, got %s" % (shape, tuple(t.shape)))
    out = torch.empty((n, N + dummy_rows, 3), dtype=torch.float32, device=raw.device)
    check(_lib.load().sh_dataset_normalize(ptr(raw), ptr(out), n, N, dummy_rows, flags, ptr(j_root), ptr(mean), ptr(std),
                                           ptr(center), ptr(scale), stream_ptr()), "sh_dataset_normalize")
    return out


def gather_meshes(src, idx):
    """src [n, ...] contiguous fp32 HIP tensor, idx int64 HIP tensor [b] -> src[idx] (bit-exact copy)."""
    if not (src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and idx.is_cuda and idx.dtype == torch.int64
            and idx.dim() == 1 and idx.is_contiguous()):
        raise RuntimeError("semantichuman_amd.gather_meshes needs a contiguous fp32 HIP tensor and an int64 HIP index; no CPU path")
    b = idx.numel()
    out = torch.empty((b,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    if b:
        check(_lib.load().sh_gather_meshes(ptr(src), src[0].numel(), ptr(idx), b, ptr(out), stream_ptr()), "sh_gather_meshes")
    return out


# ------------------------------------------------------------------------------------------ bf16 compute path
_ANY = (torch.float32, torch.bfloat16)


def dtype_id(t: torch.Tensor) -> int:
    return _lib.DTYPE_IDS[str(t.dtype).replace("torch.", "")]


def conv_wfrag_prep(weights, dims, transpose):
    """fp32 master weights [Cout, S*Cin] -> bf16 fragment-ordered working copies (uint8 buffers), one launch.
    dims: [(S, Cin, Cout)]; transpose: [0 forward operand | 1 backward-data operand]."""
    import ctypes
    lib = _lib.load()
    outs = []
    for w, (s, ci, co), tr in zip(weights, dims, transpose):
        if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()):
            raise RuntimeError("conv_wfrag_prep needs contiguous fp32 HIP weights; there is no CPU path")
        nb = lib.sh_conv_wfrag_bytes(s, co if tr else ci, ci if tr else co)
        outs.append(torch.empty(nb, dtype=torch.uint8, device=w.device))
    cols = list(zip(*dims))
    args = [_c_ptr_array(list(weights)), _c_ptr_array(outs)] + [_c_int_array(c) for c in cols] + [_c_int_array([int(t) for t in transpose])]
    check(lib.sh_conv_wfrag_prep_multi(len(outs), *[ctypes.cast(a, ctypes.c_void_p) for a in args], stream_ptr()),
          "sh_conv_wfrag_prep_multi")
    return outs


def spiral_conv_fwd_bf16(x, x_layout, table, wfrag, bias, y, y_layout, R, S, Cin, Cout, act, zero_row):
    B, _, C1, xsv, xsb = _dims(x, x_layout, _ANY)
    B2, Ry, C2, ysv, ysb = _dims(y, y_layout, _ANY)
    assert B == B2 and Ry >= R and C1 == Cin and C2 == Cout and table.dtype == torch.int32
    _check_index_range(x)
    check(_lib.load().sh_spiral_conv_fwd_bf16(ptr(x), dtype_id(x), xsv, xsb, ptr(table), ptr(wfrag), ptr(bias), ptr(y), dtype_id(y),
                                              ysv, ysb, B, R, S, Cin, Cout, act, zero_row, stream_ptr()), "sh_spiral_conv_fwd_bf16")


def spiral_conv_bwd_data_bf16(dpre, dp_layout, table_t, wfrag_t, dx, dx_layout, yprev, yp_layout, act_prev, zero_row, n_in, S, Cin, Cout):
    B, _, C1, dsv, dsb = _dims(dpre, dp_layout, _ANY)
    B2, Rx, C2, xsv, xsb = _dims(dx, dx_layout, _ANY)
    assert B == B2 and C1 == Cout and C2 == Cin and Rx >= n_in and tuple(table_t.shape) == (n_in, S)
    _check_index_range(dpre)
    if yprev is not None:
        _, _, C3, ysv, ysb = _dims(yprev, yp_layout, (torch.bfloat16,))
        assert C3 == Cin
    else:
        ysv = ysb = 0
    check(_lib.load().sh_spiral_conv_bwd_data_bf16(ptr(dpre), dtype_id(dpre), dsv, dsb, ptr(table_t), ptr(wfrag_t), ptr(dx),
                                                   dtype_id(dx), xsv, xsb, ptr(yprev), ysv, ysb, act_prev, zero_row, B, n_in, S,
                                                   Cin, Cout, stream_ptr()), "sh_spiral_conv_bwd_data_bf16")


def spiral_conv_bf16_rag_ok(B, S, Cg, Nout, rag_L) -> bool:
    return bool(_lib.load().sh_spiral_conv_bf16_rag_ok(B, S, Cg, Nout, rag_L))


def spiral_conv_bwd_data_bf16_rag(dpre, dp_layout, rag_rows, rag_pos, wfrag_t, dx, dx_layout, yprev, yp_layout, act_prev, zero_row, n_in, S,
                                  Cin, Cout):
    """Backward-data over ragged source lists (mesh_ops.transpose_table_ragged): bf16 on both sides, no pre-summed rows."""
    B, _, C1, dsv, dsb = _dims(dpre, dp_layout, (torch.bfloat16,))
    B2, Rx, C2, xsv, xsb = _dims(dx, dx_layout, (torch.bfloat16,))
    assert B == B2 and C1 == Cout and C2 == Cin and Rx >= n_in and rag_rows.shape == rag_pos.shape and rag_rows.shape[0] == n_in
    assert rag_rows.dtype == torch.int32 and rag_pos.dtype == torch.int32 and rag_rows.is_contiguous() and rag_pos.is_contiguous()
    _check_index_range(dpre)
    if yprev is not None:
        _, _, C3, ysv, ysb = _dims(yprev, yp_layout, (torch.bfloat16,))
        assert C3 == Cin
    else:
        ysv = ysb = 0
    check(_lib.load().sh_spiral_conv_bwd_data_bf16_rag(ptr(dpre), dsv, dsb, ptr(rag_rows), ptr(rag_pos), int(rag_rows.shape[1]), ptr(wfrag_t),
                                                       ptr(dx), xsv, xsb, ptr(yprev), ysv, ysb, act_prev, zero_row, B, n_in, S, Cin, Cout,
                                                       stream_ptr()), "sh_spiral_conv_bwd_data_bf16_rag")


def spiral_conv_bwd_wgt_bf16(dpre, dp_layout, x, x_layout, table, R, S, Cin, Cout, want_bias=True):
    """-> (dW fp32 [Cout, S*Cin], dbias fp32 [Cout] or None)"""
    import ctypes
    B, _, C1, dsv, dsb = _dims(dpre, dp_layout, _ANY)
    B2, _, C2, xsv, xsb = _dims(x, x_layout, _ANY)
    assert B == B2 and C1 == Cout and C2 == Cin
    lib = _lib.load()
    nbytes = lib.sh_spiral_conv_bwd_wgt_workspace_bf16(B, R, S, Cin, Cout)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    check(lib.sh_spiral_conv_bwd_wgt_bf16(ptr(dpre), dtype_id(dpre), dsv, dsb, ptr(x), dtype_id(x), xsv, xsb, ptr(table), ptr(ws), nbytes,
                                          B, R, S, Cin, Cout, stream_ptr()), "sh_spiral_conv_bwd_wgt_bf16")
    dW = torch.empty((Cout, S * Cin), dtype=torch.float32, device=x.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if want_bias else None
    args = [_c_ptr_array([ws]), _c_ptr_array([dW]), _c_ptr_array([db])] + [_c_int_array([v]) for v in (B, R, S, Cin, Cout)]
    check(lib.sh_spiral_conv_bwd_wgt_reduce_multi_bf16(1, *[ctypes.cast(a, ctypes.c_void_p) for a in args], stream_ptr()),
          "sh_spiral_conv_bwd_wgt_reduce_multi_bf16")
    return dW, db


def wgrad_thin_ok(B, n_in, S, Cin, Cout, dtype) -> bool:
    return bool(_lib.load().sh_spiral_conv_bwd_wgt_thin_ok(B, n_in, S, Cin, Cout, _lib.DTYPE_IDS[str(dtype).replace("torch.", "")]))


def _thin_dx_args(dx, weight, B, Cin, act_prev, zero_prev):
    if dx is None:
        return [None, None, 0, 0, None, 0, -1]
    _, _, Cd, gsv, gsb = _dims(dx, "vm", _ANY)
    assert Cd == Cin and weight is not None
    return [ptr(weight), ptr(dx), gsv, gsb, None, int(act_prev), int(zero_prev)]


def spiral_conv_bwd_wgt_thin_deferred(dpre_ext, x, table_t, R, S, Cin, Cout, want_bias=True, weight=None, dx=None, act_prev=0,
                                      zero_prev=-1):
    """fp32 path: slabs only; the job goes to `spiral_conv_bwd_wgt_reduce` with the other layers of the stack.
    dx (vertex-major [>= R, B, Cin]) given: the launch also writes the layer's input gradient (see sh_kernels.h)."""
    B, _, C1, dsv, dsb = _dims(dpre_ext, "vm")
    B2, rows_x, C2, xsv, xsb = _dims(x, "vm")
    assert B == B2 and C1 == Cout and C2 == Cin and rows_x >= R
    lib = _lib.load()
    nbytes = lib.sh_spiral_conv_bwd_wgt_workspace(B, R, S, Cin, Cout)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    check(lib.sh_spiral_conv_bwd_wgt_thin(ptr(dpre_ext), dsv, dsb, ptr(x), dtype_id(x), xsv, xsb, ptr(table_t), ptr(ws), nbytes,
                                          *_thin_dx_args(dx, weight, B, Cin, act_prev, zero_prev), B, R, R, S, Cin, Cout, dtype_id(x),
                                          stream_ptr()), "sh_spiral_conv_bwd_wgt_thin")
    dW = torch.empty((Cout, S * Cin), dtype=torch.float32, device=x.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if want_bias else None
    return dict(ws=ws, dW=dW, db=db, dims=(B, R, S, Cin, Cout))


def spiral_conv_bwd_wgt_thin(dpre_ext, x, table_t, R, S, Cin, Cout, want_bias=True, weight=None, dx=None, act_prev=0, zero_prev=-1):
    """Role-swapped weight gradient of a 16 -> 3 channel layer (wgrad_thin.hip): dpre_ext fp32 [rows >= R (+ pre-summed extra
    rows), B, 3] and x [R, B, 16] (fp32 or bf16: selects the path), both vertex-major; table_t int32 [R, S] the transposed
    table backward-data uses.  -> (dW fp32 [Cout, S*Cin], dbias fp32 [Cout] or None)."""
    import ctypes
    B, _, C1, dsv, dsb = _dims(dpre_ext, "vm", _ANY)
    B2, rows_x, C2, xsv, xsb = _dims(x, "vm", _ANY)
    assert B == B2 and C1 == Cout and C2 == Cin and rows_x >= R and dpre_ext.dtype == torch.float32
    lib = _lib.load()
    b16 = x.dtype == torch.bfloat16
    if not lib.sh_spiral_conv_bwd_wgt_thin_ok(B, R, S, Cin, Cout, dtype_id(x)):
        raise RuntimeError("spiral_conv_bwd_wgt_thin: shape not covered (B %d R %d S %d Cin %d Cout %d)" % (B, R, S, Cin, Cout))
    nbytes = (lib.sh_spiral_conv_bwd_wgt_workspace_bf16 if b16 else lib.sh_spiral_conv_bwd_wgt_workspace)(B, R, S, Cin, Cout)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    check(lib.sh_spiral_conv_bwd_wgt_thin(ptr(dpre_ext), dsv, dsb, ptr(x), dtype_id(x), xsv, xsb, ptr(table_t), ptr(ws), nbytes,
                                          *_thin_dx_args(dx, weight, B, Cin, act_prev, zero_prev), B, R, R, S, Cin, Cout, dtype_id(x),
                                          stream_ptr()), "sh_spiral_conv_bwd_wgt_thin")
    dW = torch.empty((Cout, S * Cin), dtype=torch.float32, device=x.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if want_bias else None
    args = [_c_ptr_array([ws]), _c_ptr_array([dW]), _c_ptr_array([db])] + [_c_int_array([v]) for v in (B, R, S, Cin, Cout)]
    red = lib.sh_spiral_conv_bwd_wgt_reduce_multi_bf16 if b16 else lib.sh_spiral_conv_bwd_wgt_reduce_multi
    check(red(1, *[ctypes.cast(a, ctypes.c_void_p) for a in args], stream_ptr()), "sh_spiral_conv_bwd_wgt_reduce_multi")
    return dW, db


def cast_bf16(src, out=None):
    """fp32 HIP tensor -> bf16 copy (one streaming kernel); `out`: an existing bf16 tensor of the same shape to refresh
    in place (its address may be baked into a captured hipGraph)."""
    if not (src.is_cuda and src.dtype == torch.float32 and src.is_contiguous()):
        raise RuntimeError("cast_bf16 needs a contiguous fp32 HIP tensor; there is no CPU path")
    if out is not None and not (out.is_cuda and out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape == src.shape
                                and out.device == src.device):
        raise RuntimeError("cast_bf16: `out` must be a contiguous bf16 HIP tensor of the source's shape and device")
    dst = out if out is not None else torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    if src.numel():
        check(_lib.load().sh_cast_f32_to_bf16(ptr(src), ptr(dst), src.numel(), stream_ptr()), "sh_cast_f32_to_bf16")
    return dst


def _check2d_any(*ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.dtype in _ANY and t.is_contiguous()):
            raise RuntimeError("semantichuman_amd bf16 linear kernels need contiguous bf16/fp32 HIP tensors (got %s %s); there is no "
                               "CPU path" % (t.device, t.dtype))


def _linear_ws_bf16(M, N, K, device):
    nbytes = _lib.load().sh_linear_workspace_bf16(M, N, K)
    return torch.empty(max(4, (nbytes + 3) // 4), dtype=torch.float32, device=device), nbytes


def linear_fwd_bf16(x, w_bf16, bias, out_dtype):
    _check2d_any(x)
    M, K = x.shape
    N = w_bf16.shape[0]
    assert w_bf16.dtype == torch.bfloat16 and w_bf16.shape[1] == K and w_bf16.is_contiguous()
    y = torch.empty((M, N), dtype=out_dtype, device=x.device)
    ws, nb = _linear_ws_bf16(M, N, K, x.device)
    check(_lib.load().sh_linear_fwd_bf16(ptr(x), dtype_id(x), ptr(w_bf16), ptr(bias), ptr(y), dtype_id(y), M, N, K, ptr(ws), nb,
                                         stream_ptr()), "sh_linear_fwd_bf16")
    return y


def linear_bwd_data_bf16(dy, w_bf16, out_dtype):
    _check2d_any(dy)
    M, N = dy.shape
    K = w_bf16.shape[1]
    dx = torch.empty((M, K), dtype=out_dtype, device=dy.device)
    ws, nb = _linear_ws_bf16(M, N, K, dy.device)
    check(_lib.load().sh_linear_bwd_data_bf16(ptr(dy), dtype_id(dy), ptr(w_bf16), ptr(dx), dtype_id(dx), M, N, K, ptr(ws), nb,
                                              stream_ptr()), "sh_linear_bwd_data_bf16")
    return dx


def linear_bwd_wgt_bf16(dy, x, want_bias=True):
    _check2d_any(dy, x)
    M, N = dy.shape
    K = x.shape[1]
    dW = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    db = torch.empty((N,), dtype=torch.float32, device=dy.device) if want_bias else None
    check(_lib.load().sh_linear_bwd_wgt_bf16(ptr(dy), dtype_id(dy), ptr(x), dtype_id(x), ptr(dW), ptr(db), M, N, K, stream_ptr()),
          "sh_linear_bwd_wgt_bf16")
    return dW, db
