"""The latent fully-connected kernels (csrc/linear.hip) and the multi-tensor Adam (csrc/adam.hip, csrc/sh_adam.h) against a plain
float64 evaluation (tests/linear_ref.py), form by form, at the smallest shapes that reach each kernel and each branch of its
launcher: the 16-row tile counts of the streaming kernels, the LDS-DMA kernels and their bf16x3 forms, split reductions with a full
and a short last range, 64-row chunks with one and two live rows, the resident-weight kernel, the three staging modes of the generic
kernel, operands one float off their 16-byte alignment, the tile weight gradient with its workgroup tail, the fused and the
stand-alone bias gradient, the fused Adam update, and the optimiser's argument table, chunk boundary, scalar path and bf16 shadow.

Every output lies inside a larger buffer and starts as NaN, together with the buffer around it and the workspace behind its
promised size: an element that is not written fails its bound, and a write outside the output is seen.  Inputs end in NaN too, so
a read past an operand poisons the result.  Every element is compared with its own bound (derived in tests/linear_ref.py); the
library's dispatch record says which kernel ran and how the reduction was split, and each case asserts the kernel it exists for."""
import ctypes
import functools
import itertools
import re

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, ops

from tests import linear_ref as L
from tests.launch_record import launches

pytestmark = pytest.mark.gpu

NAN = float("nan")
SH_OK, SH_ERR_INVALID_ARG, SH_ERR_UNSUPPORTED, SH_ERR_WORKSPACE = 0, -1, -2, -3
FORMS = ("exact", "split3")
PAD = 512                      # NaN floats before and after every input


def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------ buffers
class Out:
    """An output of `shape` inside a NaN buffer: `off` floats past a 16-byte boundary, a guard of at least 64 rows on either side."""

    def __init__(self, shape, off=0, dtype=torch.float32):
        self.n = int(np.prod(shape))
        g = max(4096, 64 * int(shape[-1]))
        self.lo = g + off
        self.buf = torch.full((g + off + self.n + g,), NAN, dtype=dtype, device=dev())
        self.t = self.buf[self.lo:self.lo + self.n].view(*shape)
        assert (self.t.data_ptr() % 16 == 0) == (off * self.buf.element_size() % 16 == 0)

    def np(self):
        return self.t.detach().float().cpu().numpy()

    def untouched(self):
        """The whole buffer is still NaN (nothing was written at all)."""
        return bool(torch.isnan(self.buf).all())

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.lo + self.n:]).all())


def put(a, off=0, dtype=torch.float32):
    """numpy array -> a contiguous device view holding it, `off` elements past a 16-byte boundary, NaN before and after."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((PAD + off + a.size + PAD,), NAN, dtype=dtype, device=dev())
    v = buf[PAD + off:PAD + off + a.size].view(*a.shape)
    v.copy_(torch.from_numpy(a).to(dtype))
    return v


class Workspace:
    """Exactly sh_linear_workspace(M, N, K) bytes (or `nbytes`), NaN behind them."""

    def __init__(self, M, N, K, nbytes=None):
        self.nbytes = int(_lib.load().sh_linear_workspace(M, N, K)) if nbytes is None else int(nbytes)
        self.words = (self.nbytes + 3) // 4
        self.buf = torch.full((self.words + 64 * max(N, K) + 4096,), NAN, dtype=torch.float32, device=dev())

    def guard_intact(self):
        return bool(torch.isnan(self.buf[self.words:]).all())


def check(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    ok = err <= bound                                       # NaN (an unwritten element, a poisoned sum) is not ok
    if not ok.all():
        e = np.where(ok, -1.0, np.nan_to_num(err, nan=np.inf))
        i = np.unravel_index(int(np.argmax(e)), err.shape)
        pytest.fail("%s: %d of %d elements outside the bound; worst at %s: got %r ref %r bound %.3e" % (
            what, int((~ok).sum()), err.size, i, float(got[i]), float(ref[i]), float(bound[i])))


def split_of(tag):
    m = re.search(r"split=(\d+)", tag)
    return int(m.group(1)) if m else 1


def main_launch(rec, kernel):
    """The record must hold `kernel`; -> its tag."""
    names = [k for k, _ in rec]
    assert kernel in names, "expected %s, the call launched %s" % (kernel, rec)
    return rec[names.index(kernel)][1]


# -------------------------------------------------------------------------------------------------------------- kernel calls
def k_fwd(x, w, b, y, M, N, K, form, ws):
    return _lib.load().sh_linear_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), M, N, K, _lib.ptr(ws.buf), ws.nbytes,
                                     _lib.mma_id(form), _lib.stream_ptr())


def k_bwd_data(dy, w, dx, M, N, K, form, ws):
    return _lib.load().sh_linear_bwd_data(_lib.ptr(dy), _lib.ptr(w), _lib.ptr(dx), M, N, K, _lib.ptr(ws.buf), ws.nbytes,
                                          _lib.mma_id(form), _lib.stream_ptr())


def k_bwd_wgt(dy, x, dW, db, M, N, K, form, ws):
    return _lib.load().sh_linear_bwd_wgt(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(dW), _lib.ptr(db), M, N, K, _lib.ptr(ws.buf), ws.nbytes,
                                         _lib.mma_id(form), _lib.stream_ptr())


def k_wgt_adam(dy, x, w, w16, m, v, step, lr, betas, eps, wd, db, M, N, K, form):
    did = lambda t: 1 if t.dtype == torch.bfloat16 else 0               # noqa: E731 - enum sh_dtype
    return _lib.load().sh_linear_bwd_wgt_adam(_lib.ptr(dy), did(dy), _lib.ptr(x), did(x), _lib.ptr(w), _lib.ptr(w16), _lib.ptr(m), _lib.ptr(v),
                                              _lib.ptr(step), _lib.ptr(lr), float(betas[0]), float(betas[1]), float(eps), float(wd),
                                              _lib.ptr(db), M, N, K, _lib.mma_id(form), _lib.stream_ptr())


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[0 if t is None else t.data_ptr() for t in ts])


def k_adam(p, g, m, v, steps, numel, lr, betas, eps, wd, shadow=None):
    """sh_adam_step (sh_adam_step_bf16 when `shadow` is a list) over lists of tensors (entries may be None) -> status."""
    lib = _lib.load()
    n = len(steps)
    N = (ctypes.c_int64 * n)(*[int(k) for k in numel])
    head = [n, _ptrs(p), _ptrs(g), _ptrs(m), _ptrs(v), _ptrs(steps)]
    tail = [N, _lib.ptr(lr), float(betas[0]), float(betas[1]), float(eps), float(wd), _lib.stream_ptr()]
    if shadow is None:
        return lib.sh_adam_step(*head, *tail)
    return lib.sh_adam_step_bf16(*head, _ptrs(shadow), *tail)


@functools.lru_cache(maxsize=None)
def ops_of(M, N, K):
    """The shared, read-only operands of a shape and their float64 references."""
    x, w, b, dy = L.operands(M, N, K, seed=L.seed_of(M, N, K))
    return dict(x=x, w=w, b=b, dy=dy, fwd=L.fwd64(x, w, b), fwd0=L.fwd64(x, w, None), bwd=L.bwd_data64(dy, w), wgt=L.bwd_wgt64(dy, x))


SEEN = set()                   # every kernel name the sweep observed (test_every_kernel_is_observed)


def note(rec):
    SEEN.update(k for k, _ in rec)


# ==================================================================================================================== forward
def S(m):
    return "linear_fwd_stream_kernel<%d>" % m


def D(m):
    return "linear_fwd_dma_kernel<%d>" % m


def X(m):
    return "linear_fwd_x3_kernel<%d>" % m


GEMM, WIDE, REDUCE, COLSUM = "skinny_gemm_kernel", "linear_fwd_wide_x3_kernel", "split_reduce_kernel", "colsum_kernel"

# (M, N, K): (kernel in the exact form, kernel in the bf16x3 forms, split, staging modes of the generic kernel or None)
FWD = {}
for _M in (1, 16, 17, 32, 33, 48, 49, 64):                 # one to four 16-row tiles, each full and with one live row; N / 64 = 1: no x3 form
    FWD[(_M, 64, 48)] = (S((_M + 15) // 16), S((_M + 15) // 16), 1, None)
for _M in (1, 17, 33, 64):                                 # four column groups and K % 32 == 0: the LDS-DMA kernel and its x3 form
    FWD[(_M, 256, 64)] = (D((_M + 15) // 16), X((_M + 15) // 16), 1, None)
FWD[(5, 64, 1024)] = (S(1), S(1), 16, None)                # sixteen full ranges of 64
FWD[(5, 64, 1040)] = (S(1), S(1), 17, None)                # ... and a last range of 16
FWD[(5, 256, 1056)] = (D(1), X(1), 17, None)               # 32-granular ranges, a last range of 32
FWD[(64, 256, 1088)] = (D(4), X(4), 17, None)
FWD[(65, 256, 416)] = (D(4), X(4), 1, None)                # 64-row chunks over gridDim.y: one live row in the last
FWD[(130, 256, 992)] = (D(4), X(4), 1, None)               # ... two live rows in the third
FWD[(65, 64, 32)] = (GEMM, WIDE, 1, "00")                  # the resident-weight kernel: M > 64, K <= 384; fp32 MFMA elsewhere
FWD[(130, 128, 384)] = (GEMM, WIDE, 1, "00")
FWD[(200, 64, 352)] = (GEMM, WIDE, 1, "00")
FWD[(5, 7, 13)] = (GEMM, GEMM, 1, "22")                    # ragged: scalar staging
FWD[(4, 8, 2048)] = (GEMM, GEMM, 8, "00")
FWD[(3, 5, 2050)] = (GEMM, GEMM, 9, "22")                  # a last chunk of 2
FWD[(65, 64, 1024)] = (GEMM, GEMM, 1, "00")
FWD[(70, 130, 96)] = (GEMM, GEMM, 1, "00")
FWD[(17, 64, 64)] = (S(2), S(2), 1, None)                  # the aligned partner of the misaligned cases below
FWD[(17, 128, 64)] = (S(2), S(2), 1, None)                 # K % 32 == 0, but two column groups: not the LDS-DMA kernel's shape
FWD[(17, 256, 48)] = (S(2), S(2), 1, None)                 # four column groups, but K % 32 != 0
FWD[(65, 256, 1024)] = (GEMM, GEMM, 1, "00")               # M > 64 with a reduction that would be split (K > 384: no resident form)
FWD_NOBIAS = [(17, 64, 48), (17, 256, 64), (5, 64, 1040), (5, 256, 1056), (65, 64, 32), (5, 7, 13), (4, 8, 2048)]
FWD_PLANES3 = [(17, 64, 48), (33, 256, 64), (5, 256, 1056), (130, 128, 384), (3, 5, 2050)]     # one case per kernel


def run_fwd(shape, form, bias=True, off=None):
    """One forward call -> nothing; asserts kernel, split, every element, the guards.  off: the operand one float off alignment."""
    M, N, K = shape
    o = ops_of(M, N, K)
    kern_exact, kern_x3, split, modes = FWD[shape]
    kern = kern_exact if form == "exact" else kern_x3
    if off is not None:
        kern, modes = GEMM, {"x": "20", "w": "02", "y": "00", "b": "00"}[off]
    x, w = put(o["x"], off == "x"), put(o["w"], off == "w")
    b = put(o["b"], off == "b") if bias else None
    y, ws = Out((M, N), off == "y"), Workspace(M, N, K)
    rc, rec = launches(lambda: k_fwd(x, w, b, y.t, M, N, K, form, ws))
    note(rec)
    what = "linear_fwd %s %s%s%s" % (shape, form, "" if bias else " no bias", " %s misaligned" % off if off else "")
    assert rc == SH_OK, "%s: status %d: %s" % (what, rc, _lib.load().sh_last_error())
    tag = main_launch(rec, kern)
    assert split_of(tag) == split, "%s: %s" % (what, rec)
    assert (REDUCE in [k for k, _ in rec]) == (split > 1), rec
    if kern == GEMM:
        assert tag.endswith("modes=" + modes), "%s: %s" % (what, tag)
    ref, absum = o["fwd"] if bias else o["fwd0"]
    check(y.np(), ref, L.sum_bound(absum, K, x3="x3" in kern, split=split), what)
    assert y.guards_intact() and ws.guard_intact(), "%s: a write outside the output or the workspace" % what
    if off is None:                                          # the wrapper the layers call: the same kernel, the same bits
        yo = ops.linear_fwd(x, w, b, mma=form)
        assert L.same_bits(yo.cpu().numpy(), y.np()), what
    return split, ws


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", list(FWD), ids=lambda s: "%dx%dx%d" % s)
def test_forward(shape, form):
    run_fwd(shape, form)


@pytest.mark.parametrize("shape", FWD_PLANES3, ids=lambda s: "%dx%dx%d" % s)
def test_forward_planes3(shape):
    run_fwd(shape, "planes3")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", FWD_NOBIAS, ids=lambda s: "%dx%dx%d" % s)
def test_forward_without_bias(shape, form):
    run_fwd(shape, form, bias=False)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("off", ["x", "w", "y", "b"])
def test_forward_misaligned_operand_takes_the_generic_kernel(off, form):
    run_fwd((17, 64, 64), form, off=off)


# ============================================================================================================== backward-data
def BS(m):
    return "linear_bwd_data_stream_kernel<%d>" % m


def BX(m):
    return "linear_bwd_data_x3_kernel<%d>" % m


BWD = {}                                                   # (M, N, K): out = K, reduction = N
for _M in (1, 16, 17, 32, 33, 48, 49, 64):
    BWD[(_M, 48, 64)] = (BS((_M + 15) // 16), BS((_M + 15) // 16), 1, None)          # N % 32 != 0: no x3 form
for _M in (1, 17, 33, 64):
    BWD[(_M, 96, 64)] = (BS((_M + 15) // 16), BX((_M + 15) // 16), 1, None)
BWD[(5, 1024, 64)] = (BS(1), BX(1), 16, None)
BWD[(5, 1040, 64)] = (BS(1), BS(1), 17, None)              # a last range of 16 (which the 32-row x3 steps cannot take)
BWD[(33, 1056, 256)] = (BS(3), BX(3), 17, None)            # a last range of 32
BWD[(5, 13, 8)] = (GEMM, GEMM, 1, "21")                    # the weight staged along its contiguous output index
BWD[(5, 13, 7)] = (GEMM, GEMM, 1, "22")
BWD[(65, 64, 64)] = (GEMM, GEMM, 1, "01")
BWD[(3, 2050, 5)] = (GEMM, GEMM, 9, "22")
BWD[(17, 64, 64)] = (BS(2), BX(2), 1, None)
BWD_PLANES3 = [(17, 48, 64), (33, 96, 64), (33, 1056, 256), (5, 13, 8)]


def run_bwd_data(shape, form, off=None):
    M, N, K = shape
    o = ops_of(M, N, K)
    kern_exact, kern_x3, split, modes = BWD[shape]
    kern = kern_exact if form == "exact" else kern_x3
    if off is not None:
        kern, modes = GEMM, {"dy": "21", "w": "02", "dx": "01"}[off]
    dy, w = put(o["dy"], off == "dy"), put(o["w"], off == "w")
    dx, ws = Out((M, K), off == "dx"), Workspace(M, N, K)
    rc, rec = launches(lambda: k_bwd_data(dy, w, dx.t, M, N, K, form, ws))
    note(rec)
    what = "linear_bwd_data %s %s%s" % (shape, form, " %s misaligned" % off if off else "")
    assert rc == SH_OK, "%s: status %d: %s" % (what, rc, _lib.load().sh_last_error())
    tag = main_launch(rec, kern)
    assert split_of(tag) == split, "%s: %s" % (what, rec)
    assert (REDUCE in [k for k, _ in rec]) == (split > 1), rec
    if kern == GEMM:
        assert tag.endswith("modes=" + modes), "%s: %s" % (what, tag)
    ref, absum = o["bwd"]
    check(dx.np(), ref, L.sum_bound(absum, N, x3="x3" in kern, split=split), what)
    assert dx.guards_intact() and ws.guard_intact(), "%s: a write outside the output or the workspace" % what
    if off is None:
        assert L.same_bits(ops.linear_bwd_data(dy, w, mma=form).cpu().numpy(), dx.np()), what
    return split


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", list(BWD), ids=lambda s: "%dx%dx%d" % s)
def test_backward_data(shape, form):
    run_bwd_data(shape, form)


@pytest.mark.parametrize("shape", BWD_PLANES3, ids=lambda s: "%dx%dx%d" % s)
def test_backward_data_planes3(shape):
    run_bwd_data(shape, "planes3")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("off", ["dy", "w", "dx"])
def test_backward_data_misaligned_operand_takes_the_generic_kernel(off, form):
    run_bwd_data((17, 64, 64), form, off=off)


# ============================================================================================================ weight gradient
TILE, TILE_X3 = "linear_bwd_wgt_dma_kernel", "linear_bwd_wgt_x3_kernel"
WGT_TILE = [(1, 64, 64), (17, 64, 320), (33, 192, 64), (64, 128, 256), (64, 64, 576)]    # K / 64 = 5 and 9: a tail workgroup of one wave
WGT_GEMM = {(65, 64, 64): (1, "11"), (5, 7, 13): (1, "22"), (16, 64, 96): (1, "11"), (2048, 64, 64): (8, "11"), (17, 64, 64): (1, "11")}
DBIAS = ("aligned", "offset", "absent")


def run_bwd_wgt(shape, form, dbias, dw_off=False):
    M, N, K = shape
    o = ops_of(M, N, K)
    tile = shape in WGT_TILE and not dw_off
    kern = (TILE if form == "exact" else TILE_X3) if tile else GEMM
    split, modes = (1, None) if tile else WGT_GEMM[shape]
    dy, x = put(o["dy"]), put(o["x"])
    dW, ws = Out((N, K), int(dw_off)), Workspace(M, N, K)
    db = None if dbias == "absent" else Out((N,), int(dbias == "offset"))
    rc, rec = launches(lambda: k_bwd_wgt(dy, x, dW.t, None if db is None else db.t, M, N, K, form, ws))
    note(rec)
    what = "linear_bwd_wgt %s %s dbias %s%s" % (shape, form, dbias, " dW misaligned" if dw_off else "")
    assert rc == SH_OK, "%s: status %d: %s" % (what, rc, _lib.load().sh_last_error())
    tag = main_launch(rec, kern)
    names = [k for k, _ in rec]
    assert split_of(tag) == split and (REDUCE in names) == (split > 1), "%s: %s" % (what, rec)
    if modes is not None:
        assert tag.endswith("modes=" + modes), "%s: %s" % (what, tag)
    # the bias gradient is fused into the tile kernel when it is 16-byte aligned; otherwise, and beside the generic kernel, it is
    # colsum_kernel's
    assert (COLSUM in names) == (db is not None and (dbias == "offset" or not tile)), "%s: %s" % (what, rec)
    refW, abW, refb, abb = o["wgt"]
    check(dW.np(), refW, L.sum_bound(abW, M, x3="x3" in kern, split=split), what)
    assert dW.guards_intact() and ws.guard_intact(), "%s: a write outside the output or the workspace" % what
    if db is not None:
        check(db.np(), refb, L.sum_bound(abb, M), what + " (dbias)")
        assert db.guards_intact(), "%s: a write outside dbias" % what
    if not dw_off and dbias != "offset":
        gW, gb = ops.linear_bwd_wgt(dy, x, want_bias=db is not None, mma=form)
        assert L.same_bits(gW.cpu().numpy(), dW.np()) and (db is None or L.same_bits(gb.cpu().numpy(), db.np())), what
    return split


@pytest.mark.parametrize("dbias", DBIAS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", WGT_TILE, ids=lambda s: "%dx%dx%d" % s)
def test_weight_gradient_tile_kernel(shape, form, dbias):
    run_bwd_wgt(shape, form, dbias)


def test_weight_gradient_tile_kernel_planes3():
    run_bwd_wgt((17, 64, 320), "planes3", "aligned")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", [s for s in WGT_GEMM if s != (17, 64, 64)], ids=lambda s: "%dx%dx%d" % s)
def test_weight_gradient_generic_kernel(shape, form):
    run_bwd_wgt(shape, form, "aligned")


@pytest.mark.parametrize("form", FORMS + ("planes3",))
def test_weight_gradient_misaligned_dw_takes_the_generic_kernel(form):
    run_bwd_wgt((17, 64, 64), form, "aligned", dw_off=True)


# ========================================================================================================= workspace contract
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["fwd", "bwd_data", "bwd_wgt"])
def test_a_workspace_one_byte_short_is_refused_before_anything_is_launched(which, form):
    """The split a first call recorded says how many slabs the reduction needs; one byte fewer: SH_ERR_WORKSPACE, nothing launched,
    nothing written."""
    shape = {"fwd": (5, 256, 1056), "bwd_data": (33, 1056, 256), "bwd_wgt": (2048, 64, 64)}[which]
    M, N, K = shape
    o = ops_of(M, N, K)
    rows, cols = {"fwd": (M, N), "bwd_data": (M, K), "bwd_wgt": (N, K)}[which]
    split = {"fwd": lambda: run_fwd(shape, form)[0], "bwd_data": lambda: run_bwd_data(shape, form),
             "bwd_wgt": lambda: run_bwd_wgt(shape, form, "aligned")}[which]()
    assert split > 1
    need = split * rows * cols * 4
    assert need <= int(_lib.load().sh_linear_workspace(M, N, K))
    out, db = Out((rows, cols)), Out((N,))
    a, b, bias = (put(o["x"]), put(o["w"]), put(o["b"])) if which == "fwd" else (put(o["dy"]), put(o["w"]), None) if which == "bwd_data" else \
        (put(o["dy"]), put(o["x"]), None)
    for nbytes, want in ((need - 1, SH_ERR_WORKSPACE), (need, SH_OK)):
        ws = Workspace(M, N, K, nbytes=nbytes)
        call = {"fwd": lambda: k_fwd(a, b, bias, out.t, M, N, K, form, ws), "bwd_data": lambda: k_bwd_data(a, b, out.t, M, N, K, form, ws),
                "bwd_wgt": lambda: k_bwd_wgt(a, b, out.t, db.t, M, N, K, form, ws)}[which]
        rc, rec = launches(call)
        assert rc == want, "%s %s with %d of %d bytes: status %d" % (which, shape, nbytes, need, rc)
        if want == SH_ERR_WORKSPACE:
            assert rec == [] and out.untouched() and db.untouched() and bool(torch.isnan(ws.buf).all()), rec
        else:                                                 # exactly what the split needs is enough
            assert not torch.isnan(out.t).any() and out.guards_intact() and ws.guard_intact()


# ================================================================================================= fused weight-gradient Adam
ADAM_TILE = [(1, 64, 64), (17, 64, 320), (33, 192, 64), (64, 128, 256)]
BETAS, EPS, LR = (0.9, 0.999), 1e-8, 1e-3


def adam_tensors(N, K, step, seed, shadow):
    """Device state of one [N][K] parameter: (weight, exp_avg, exp_avg_sq, step scalar, lr scalar, bf16 shadow or None)."""
    p, _, m, v = L.adam_state(N * K, seed, step)
    t = [torch.tensor(a.reshape(N, K), device=dev()) for a in (p, m, v)]
    w16 = torch.full((N, K), NAN, dtype=torch.bfloat16, device=dev()) if shadow else None
    return t + [torch.tensor([float(step)], device=dev()), torch.tensor([LR], dtype=torch.float32, device=dev()), w16]


def bits(t):
    a = t.detach().cpu()
    return (a.view(torch.int16) if a.dtype == torch.bfloat16 else a).numpy()


@pytest.mark.parametrize("wd", [0.0, 5e-5])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", ADAM_TILE, ids=lambda s: "%dx%dx%d" % s)
def test_fused_weight_gradient_adam_is_the_two_kernel_form_bit_for_bit(shape, form, wd):
    """sh_linear_bwd_wgt_adam against sh_linear_bwd_wgt followed by sh_adam_step(_bf16) on clones: weight, both moments, dbias and
    shadow bit for bit, the step count untouched.  Both sides are anchored in float64: the gradient by the weight-gradient sweep
    above, the update by the Adam sweep below."""
    M, N, K = shape
    o = ops_of(M, N, K)
    dy, x = put(o["dy"]), put(o["x"])
    kern = "linear_bwd_wgt_adam_kernel" if form == "exact" else "linear_bwd_wgt_adam_x3_kernel"
    for step, shadow, dbias in itertools.product((0, 1, 999), (False, True), DBIAS):
        what = "%s %s wd=%g step=%d shadow=%s dbias=%s" % (shape, form, wd, step, shadow, dbias)
        w, m, v, st, lr, w16 = adam_tensors(N, K, step, seed=step + 7, shadow=shadow)
        w2, m2, v2, st2 = w.clone(), m.clone(), v.clone(), st.clone()
        w16_2 = w16.clone() if shadow else None
        db = None if dbias == "absent" else Out((N,), int(dbias == "offset"))
        rc, rec = launches(lambda: k_wgt_adam(dy, x, w, w16, m, v, st, lr, BETAS, EPS, wd, None if db is None else db.t, M, N, K, form))
        note(rec)
        assert rc == SH_OK, "%s: status %d: %s" % (what, rc, _lib.load().sh_last_error())
        main_launch(rec, kern)
        assert (COLSUM in [k for k, _ in rec]) == (dbias == "offset"), "%s: %s" % (what, rec)
        assert float(st) == float(step), what
        # the two-kernel form
        dW, ws = Out((N, K)), Workspace(M, N, K)
        db2 = None if dbias == "absent" else Out((N,), int(dbias == "offset"))
        assert k_bwd_wgt(dy, x, dW.t, None if db2 is None else db2.t, M, N, K, form, ws) == SH_OK
        assert k_adam([w2], [dW.t], [m2], [v2], [st2], [N * K], lr, BETAS, EPS, wd, [w16_2] if shadow else None) == SH_OK
        torch.cuda.synchronize()
        assert float(st2) == float(step + 1)
        for name, a, b in (("weight", w, w2), ("exp_avg", m, m2), ("exp_avg_sq", v, v2)):
            assert not torch.isnan(a).any() and L.same_bits(bits(a), bits(b)), "%s: %s differs" % (what, name)
        if shadow:
            assert L.same_bits(bits(w16), bits(w16_2)), "%s: shadow differs" % what
            assert np.array_equal(bits(w16).view(np.uint16), L.bf16_bits(w.cpu().numpy())), "%s: shadow is not rne_bf16(weight)" % what
        if db is not None:
            assert L.same_bits(db.np(), db2.np()) and db.guards_intact(), "%s: dbias differs" % what
            check(db.np(), o["wgt"][2], L.sum_bound(o["wgt"][3], M), what + " (dbias)")


@pytest.mark.parametrize("which", ["dy", "x", "both"])
@pytest.mark.parametrize("shape", [(1, 64, 64), (17, 64, 320)], ids=lambda s: "%dx%dx%d" % s)
def test_fused_adam_with_bf16_operands_is_the_fp32_kernel_on_the_widened_tensors(shape, which):
    M, N, K = shape
    x, w_, b_, dy = L.operands(M, N, K, seed=77, bf16=True)
    f32 = {"dy": put(dy), "x": put(x)}
    b16 = {"dy": put(dy, dtype=torch.bfloat16), "x": put(x, dtype=torch.bfloat16)}
    assert np.array_equal(b16["dy"].float().cpu().numpy(), dy)
    pick = lambda k: b16[k] if which in (k, "both") else f32[k]           # noqa: E731
    got, ref = [], []
    for out, a_dy, a_x in ((got, pick("dy"), pick("x")), (ref, f32["dy"], f32["x"])):
        w, m, v, st, lr, w16 = adam_tensors(N, K, 7, seed=5, shadow=True)
        db = Out((N,))
        rc, rec = launches(lambda: k_wgt_adam(a_dy, a_x, w, w16, m, v, st, lr, BETAS, EPS, 5e-5, db.t, M, N, K, "exact"))
        note(rec)
        assert rc == SH_OK, _lib.load().sh_last_error()
        tag = main_launch(rec, "linear_bwd_wgt_adam_kernel")
        if out is got:
            assert "dy=%s x=%s" % ("bf16" if which in ("dy", "both") else "f32", "bf16" if which in ("x", "both") else "f32") in tag, tag
        else:
            assert "dy=" not in tag, tag
        out.extend([w, m, v, w16, db.t.clone()])
        assert float(st) == 7.0 and db.guards_intact()
    for name, a, b in zip(("weight", "exp_avg", "exp_avg_sq", "shadow", "dbias"), got, ref):
        assert not torch.isnan(a.float()).any() and L.same_bits(bits(a), bits(b)), "%s %s: %s differs" % (shape, which, name)


REFUSALS = {
    "M=65": dict(shape=(65, 64, 64), rc=SH_ERR_UNSUPPORTED),
    "N=96": dict(shape=(17, 96, 64), rc=SH_ERR_UNSUPPORTED),
    "K=96": dict(shape=(17, 64, 96), rc=SH_ERR_UNSUPPORTED),
    "misaligned moment": dict(shape=(17, 64, 64), rc=SH_ERR_UNSUPPORTED, moment_off=True),
    "bf16 dy, offset dbias": dict(shape=(17, 64, 64), rc=SH_ERR_UNSUPPORTED, dy16=True, db_off=True),
    "beta2=1": dict(shape=(17, 64, 64), rc=SH_ERR_INVALID_ARG, betas=(0.9, 1.0)),
    "eps<0": dict(shape=(17, 64, 64), rc=SH_ERR_INVALID_ARG, eps=-1e-8),
}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(REFUSALS))
def test_fused_adam_refusals_launch_nothing_and_change_nothing(case, form):
    c = REFUSALS[case]
    M, N, K = c["shape"]
    x, _, _, dy = L.operands(M, N, K, seed=3, bf16=c.get("dy16", False))
    dy, x = put(dy, dtype=torch.bfloat16 if c.get("dy16") else torch.float32), put(x)
    p, _, m, v = L.adam_state(N * K, 4, 7)
    w, mm, vv = put(p.reshape(N, K)), put(m.reshape(N, K), off=int(c.get("moment_off", False))), put(v.reshape(N, K))
    st, lr = torch.tensor([7.0], device=dev()), torch.tensor([LR], dtype=torch.float32, device=dev())
    w16, db = Out((N, K), dtype=torch.bfloat16), Out((N,), int(c.get("db_off", False)))
    before = [bits(t).copy() for t in (w, mm, vv, st)]
    rc, rec = launches(lambda: k_wgt_adam(dy, x, w, w16.t, mm, vv, st, lr, c.get("betas", BETAS), c.get("eps", EPS), 5e-5, db.t, M, N, K, form))
    assert rc == c["rc"], "%s: status %d: %s" % (case, rc, _lib.load().sh_last_error())
    assert rec == [], rec
    assert all(L.same_bits(a, bits(t)) for a, t in zip(before, (w, mm, vv, st))) and w16.untouched() and db.untouched(), case


# ===================================================================================================== multi-tensor Adam
NUMELS = (1, 3, 255, 4095, 4096, 4097, 8197)      # below, at and above the 4096-element chunk; a ragged second and third chunk
STEPS = (0, 1, 7, 999)
ALL_BETAS = [(0.9, 0.999), (0.5, 0.999), (0.0, 0.5)]         # w = 1 - beta1 below, at and above the 0.5 at which lerp switches its form


class AdamTensor:
    """One entry of a launch: p / g / m / v as views with NaN around them (p one float off alignment when asked), its own step."""

    def __init__(self, numel, step, seed, p_off=False, shadow=False, null=False):
        self.numel, self.step = numel, step
        n = max(numel, 8)                                     # a numel == 0 entry still owns memory: it must stay as it is
        self.host = L.adam_state(n, seed, step, zero_grad_at=(0, 2, 4095, 4096, n - 1))
        self.null = null
        self.dev = [put(a, off=int(p_off and i == 0)) for i, a in enumerate(self.host)]
        self.before = [bits(t).copy() for t in self.dev]
        self.st = torch.tensor([float(step)], device=dev())
        self.w16 = Out((n,), dtype=torch.bfloat16) if shadow else None

    def args(self):
        return [None] * 4 if self.null else self.dev

    def verify(self, lr, betas, eps, wd, what):
        what = "%s numel=%d step=%d" % (what, self.numel, self.step)
        assert float(self.st) == float(self.step + 1), "%s: step count %r" % (what, float(self.st))
        k = self.numel
        p, g, m, v = self.host
        assert L.same_bits(bits(self.dev[1]), self.before[1]), "%s: the gradient was written" % what
        for i in (0, 2, 3):                                  # nothing past the entry's element count is touched, nor the NaN around it
            assert L.same_bits(bits(self.dev[i])[k:], self.before[i][k:]), "%s: written past numel" % what
            base = self.dev[i]._base
            assert int(torch.isnan(base).sum()) == base.numel() - self.dev[i].numel(), "%s: written outside the tensor" % what
        if k == 0:
            assert self.w16 is None or self.w16.untouched(), "%s: the shadow of an empty entry was written" % what
            return
        ref = L.adam64(p[:k], g[:k], m[:k], v[:k], self.step, lr, betas[0], betas[1], eps, wd)
        for name, t in (("p", self.dev[0]), ("m", self.dev[2]), ("v", self.dev[3])):
            got = t.cpu().numpy()[:k]
            assert np.isfinite(got).all(), "%s: %s is not finite" % (what, name)
            check(got, ref[name][0], ref[name][1], "%s %s" % (what, name))
        if self.w16 is not None:
            got16 = bits(self.w16.t).view(np.uint16)
            assert np.array_equal(got16[:k], L.bf16_bits(self.dev[0].cpu().numpy()[:k])), "%s: shadow is not rne_bf16 of the new weight" % what
            assert self.w16.guards_intact() and bool(torch.isnan(self.w16.t[k:]).all()), "%s: shadow written past numel" % what


def launch_adam(ts, betas, wd, shadow=False):
    lr = torch.tensor([LR], dtype=torch.float32, device=dev())
    cols = list(zip(*[t.args() for t in ts]))
    rc, rec = launches(lambda: k_adam(cols[0], cols[1], cols[2], cols[3], [t.st for t in ts], [t.numel for t in ts], lr, betas, EPS, wd,
                                      [None if t.w16 is None else t.w16.t for t in ts] if shadow else None))
    note(rec)
    assert rc == SH_OK, _lib.load().sh_last_error()
    return rec, np.float32(LR)


@pytest.mark.parametrize("wd", [0.0, 5e-5])
@pytest.mark.parametrize("betas", ALL_BETAS, ids=lambda b: "b%g_%g" % b)
@pytest.mark.parametrize("p_off", [False, True], ids=["aligned", "p_offset"])
def test_adam_sizes_around_the_chunk_boundary(p_off, betas, wd):
    """One launch over every size, each with its own step count; `p` one float off alignment sends full chunks down the scalar path.
    The gradients hold exact zeros where exp_avg_sq is zero: the update divides by eps alone and stays finite."""
    ts = [AdamTensor(n, STEPS[i % 4], seed=10 * i + 1, p_off=p_off) for i, n in enumerate(NUMELS)]
    rec, lr = launch_adam(ts, betas, wd)
    tag = main_launch(rec, "adam_kernel")
    blocks = sum((n + 4095) // 4096 for n in NUMELS)
    assert "tensors=%d blocks=%d numel=%d" % (len(NUMELS), blocks, sum(NUMELS)) in tag, tag
    for t in ts:
        t.verify(lr, betas, EPS, wd, "adam %s wd=%g %s" % (betas, wd, "p offset" if p_off else "aligned"))


@pytest.mark.parametrize("count", [1, 60, 61, 125])
def test_adam_argument_table_and_empty_entries(count):
    """Up to, at and past the 60-entry argument table (one, two and three launches), every entry with its own size and step count,
    numel == 0 entries in between (null tensors, or tensors that must stay as they are): only their step counts advance."""
    sizes = (4097, 0, 3, 255, 0, 1, 4096)
    ts = []
    for i in range(count):
        n = sizes[i % len(sizes)] if count > 1 else 4097
        ts.append(AdamTensor(n, STEPS[(i + i // 4) % 4], seed=i + 1, null=(n == 0 and i % 2 == 1)))
    rec, lr = launch_adam(ts, (0.9, 0.999), 5e-5)
    # one update launch per 60 entries that hold anything (entry 60 of 61 is empty: its launch is the step bump alone)
    assert [k for k, _ in rec].count("adam_kernel") == sum(any(t.numel for t in ts[i:i + 60]) for i in range(0, count, 60)), rec
    assert ([k for k, _ in rec].count("adam_kernel"), ts[60].numel if count == 61 else 0) == ({1: 1, 60: 1, 61: 1, 125: 3}[count], 0)
    for i, t in enumerate(ts):
        t.verify(lr, (0.9, 0.999), EPS, 5e-5, "adam table of %d, entry %d" % (count, i))


def test_adam_only_empty_entries_launches_no_update_kernel():
    ts = [AdamTensor(0, s, seed=s + 1, null=bool(s & 1)) for s in STEPS]
    rec, lr = launch_adam(ts, (0.9, 0.999), 0.0)
    assert rec == [], rec
    for t in ts:
        t.verify(lr, (0.9, 0.999), EPS, 0.0, "adam, empty entries only")


@pytest.mark.parametrize("p_off", [False, True], ids=["aligned", "p_offset"])
def test_adam_bf16_shadow_on_the_vector_part_and_the_tail(p_off):
    ts = [AdamTensor(n, s, seed=n, p_off=p_off, shadow=True) for n, s in ((4097, 1), (8197, 999), (0, 7), (3, 0))]
    rec, lr = launch_adam(ts, (0.9, 0.999), 5e-5, shadow=True)
    main_launch(rec, "adam_kernel")
    for t in ts:
        t.verify(lr, (0.9, 0.999), EPS, 5e-5, "adam bf16 shadow")


def test_adam_bump_advances_61_step_counts_and_nothing_else():
    buf = torch.full((64,), NAN, device=dev())
    buf[1:62] = torch.arange(61, dtype=torch.float32, device=dev()) * 3.0
    steps = [buf[1 + i:2 + i] for i in range(61)]
    assert _lib.load().sh_adam_bump(61, _ptrs(steps), _lib.stream_ptr()) == SH_OK
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[1:62], np.arange(61, dtype=np.float32) * 3.0 + 1.0)
    assert np.isnan(got[0]) and np.isnan(got[62:]).all()


# ============================================================================================================== the record
def test_every_kernel_is_observed():
    """One pass over the case tables (on its own, whatever else of this file ran): all nine kernels of csrc/linear.hip, in each of
    their recorded forms, and the optimiser's, appear in the dispatch record."""
    SEEN.clear()
    for form in FORMS:
        for shape in FWD:
            run_fwd(shape, form)
        for shape in BWD:
            run_bwd_data(shape, form)
        for shape in WGT_TILE:
            run_bwd_wgt(shape, form, "offset")
        M, N, K = 17, 64, 320
        o = ops_of(M, N, K)
        w, m, v, st, lr, _ = adam_tensors(N, K, 1, seed=2, shadow=False)
        rc, rec = launches(lambda: k_wgt_adam(put(o["dy"]), put(o["x"]), w, None, m, v, st, lr, BETAS, EPS, 0.0, None, M, N, K, form))
        assert rc == SH_OK
        note(rec)
    run_bwd_wgt((2048, 64, 64), "exact", "aligned")
    launch_adam([AdamTensor(4097, 1, seed=1)], (0.9, 0.999), 0.0)
    want = {GEMM, REDUCE, COLSUM, WIDE, TILE, TILE_X3, "linear_bwd_wgt_adam_kernel", "linear_bwd_wgt_adam_x3_kernel", "adam_kernel"}
    want |= {f(m) for f in (S, D, X, BS, BX) for m in (1, 2, 3, 4)}
    assert want <= SEEN, "never launched: %s" % sorted(want - SEEN)
    print("kernels observed:", ", ".join(sorted(SEEN)))
