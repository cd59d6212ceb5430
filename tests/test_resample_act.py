"""The mesh re-sampling kernels (sh_spmm, sh_spmm_p3: csrc/spmm_loss.hip; sh_spmm_bf16: csrc/bf16_misc.hip) and the activation-backward
kernels (sh_act_backward, sh_act_backward_tr, sh_act_backward_tr_img: csrc/spiral_conv.hip; sh_act_backward_bf16: csrc/bf16_misc.hip)
against a plain float64 evaluation (tests/resample_ref.py), at the smallest shapes that reach each branch of each kernel: one and two
256-element parts of a row with a ragged last part, the 4- and 2-entry unrolls with every remainder, an empty row, the activation
epilogue, the zeroed row, the grid-stride wrap, the scalar forms reached through the channel count, the alignment or a stride, the
eight-channel image form, the LDS tile-turning form at and past its limits, the weight-transpose riders and the plane images.

Every comparison covers every element of the output; outputs start as NaN, so an element that is not written fails its bound.  The
bounds are derived in tests/resample_ref.py; where the arithmetic is exact (row selects, the empty row, the zeroed row, identity and
ReLU backward) the bits are compared.  The library's profiler says which kernel a launch ran; sh_act_backward has no profiler scope,
so its tests restate the launcher's rule beside each shape."""
import ctypes
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, ops

from tests import resample_ref as R
from tests.p3_ref import SH_ERR_UNSUPPORTED, arr, has_image, to_p3

pytestmark = pytest.mark.gpu

NAN = float("nan")
SH_ERR_INVALID_ARG = -1
ROWS, COLS = 27, 17
LAYS = ("vm", "bm")


def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------ layouts
def strides(lay, n, B, C):
    """(row stride, batch stride) in elements of a contiguous tensor of n rows: 'vm' [n][B][C], 'bm' [B][n][C]."""
    return (C, n * C) if lay == "bm" else (B * C, C)


def put(a, lay, dtype=torch.float32):
    """Logical [n][B][C] numpy (values already representable in dtype) -> contiguous device tensor in the layout."""
    t = torch.tensor(np.asarray(a, dtype=np.float32))               # a copy: the shared operands stay read-only
    if lay == "bm":
        t = t.permute(1, 0, 2).contiguous()
    return t.to(dtype).to(dev())


def blank(n, B, C, lay, dtype=torch.float32):
    return torch.full((B, n, C) if lay == "bm" else (n, B, C), NAN, dtype=dtype, device=dev())


def get(t, lay):
    """Device tensor in the layout -> logical [n][B][C] fp32 numpy."""
    t = t.detach().float().cpu()
    if lay == "bm":
        t = t.permute(1, 0, 2)
    return np.ascontiguousarray(t.numpy())


def worst(got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bound)                              # NaN (an unwritten element) is bad
    i = np.unravel_index(int(np.argmax(np.where(bad, np.nan_to_num(err, nan=np.inf), -1.0))), err.shape)
    return "%d of %d elements outside the bound; worst at %s: got %r ref %r bound %.3e" % (
        int(bad.sum()), err.size, i, float(got[i]), float(ref[i]), float(bound[i]))


def check(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), "%s: %s" % (what, worst(got, ref, bound))


# -------------------------------------------------------------------------------------------------------------- kernel calls
def k_spmm(bf16, csr, x, xs, y, ys, yp, yps, act, zr, B, rows, C):
    """sh_spmm / sh_spmm_bf16 on tensors (or views) with explicit (row, batch) element strides -> status."""
    lib = _lib.load()
    fn = lib.sh_spmm_bf16 if bf16 else lib.sh_spmm
    return fn(_lib.ptr(csr[0]), _lib.ptr(csr[1]), _lib.ptr(csr[2]), _lib.ptr(x), xs[0], xs[1], _lib.ptr(y), ys[0], ys[1],
              _lib.ptr(yp), yps[0], yps[1], act, zr, B, rows, C, _lib.stream_ptr())


def k_spmm_p3(csr, x, y, img, yp, act, zr, B, rows, C):
    """sh_spmm_p3 on vertex-major contiguous tensors; y or yp may be None."""
    return _lib.load().sh_spmm_p3(_lib.ptr(csr[0]), _lib.ptr(csr[1]), _lib.ptr(csr[2]), _lib.ptr(x), B * C, C, _lib.ptr(y), B * C, C,
                                  _lib.ptr(img), _lib.ptr(yp), B * C if yp is not None else 0, C if yp is not None else 0, act, zr,
                                  B, rows, C, _lib.stream_ptr())


def k_act(bf16, dy, dys, y, ys, dp, dps, B, Rn, C, act, zr):
    lib = _lib.load()
    fn = lib.sh_act_backward_bf16 if bf16 else lib.sh_act_backward
    return fn(_lib.ptr(dy), dys[0], dys[1], _lib.ptr(y), ys[0], ys[1], _lib.ptr(dp), dps[0], dps[1], B, Rn, C, act, zr, _lib.stream_ptr())


def _riders(weights, outs, dims):
    cols = list(zip(*dims))
    a = [arr([w.data_ptr() for w in weights], ctypes.c_void_p), arr([w.data_ptr() for w in outs], ctypes.c_void_p)]
    a += [arr(list(c), ctypes.c_int) for c in cols]
    return [ctypes.cast(v, ctypes.c_void_p) for v in a]


def k_act_tr(dy, dys, y, ys, dp, dps, B, Rn, C, act, zr, weights, outs, dims, img=None, with_img=False):
    """sh_act_backward_tr (or _tr_img when with_img) with the weight-transpose riders `weights` -> `outs` of dims [(S, Cin, Cout)]."""
    lib = _lib.load()
    rid = _riders(weights, outs, dims) if weights else [ctypes.c_void_p(0)] * 5
    head = [_lib.ptr(dy), dys[0], dys[1], _lib.ptr(y), ys[0], ys[1], _lib.ptr(dp), dps[0], dps[1]]
    tail = [B, Rn, C, act, zr, len(weights)] + rid + [_lib.stream_ptr()]
    if with_img:
        return lib.sh_act_backward_tr_img(*(head + [_lib.ptr(img)] + tail))
    return lib.sh_act_backward_tr(*(head + tail))


class profiled:
    """The library profiler's records of the launches made inside the block: .recs = [(kernel, tag)]."""

    def __enter__(self):
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        self.recs = []
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        try:
            if exc[0] is None:
                self.recs = [(n, tag) for n, tag, _ in _lib.profile_records_by_kernel()]
        finally:
            _lib.profile_enable(False)
        return False


# ------------------------------------------------------------------------------------------------------- shared references
@functools.lru_cache(maxsize=None)
def spmm_case(rows, cols, B, C, bf16):
    """Operands (rounded to the kernel's input type) and the float64 sums of one spmm shape, computed once and never changed."""
    rng = np.random.default_rng(1000 * rows + 10 * B + C + (5 if bf16 else 0))
    rowptr, col, val = R.make_csr(rows, cols, seed=rows + cols)
    x = R.normal((cols, B, C), rng, bf16)
    s, absum = R.spmm64(rowptr, col, val, x)
    yprev = {a: R.act_output(a, (rows, B, C), rng, bf16) for a in R.ACTS}
    for a in (x, s, absum) + tuple(yprev.values()):
        a.setflags(write=False)
    cnt = R.row_counts(rowptr)
    return SimpleNamespace(rows=rows, cols=cols, B=B, C=C, rowptr=rowptr, col=col, val=val, x=x, s=s, absum=absum, yprev=yprev,
                           empty=np.flatnonzero(cnt == 0), select=R.select_rows(rowptr, val))


def csr_dev(c):
    return tuple(torch.from_numpy(a).to(dev()) for a in (c.rowptr, c.col, c.val))


@functools.lru_cache(maxsize=None)
def act_case(B, Rn, C, bf16):
    rng = np.random.default_rng(7000 + 100 * B + 10 * Rn + C + (5 if bf16 else 0))
    dy = R.normal((Rn, B, C), rng, bf16)
    y = {a: R.act_output(a, (Rn, B, C), rng, bf16) for a in R.ACTS}
    for a in (dy,) + tuple(y.values()):
        a.setflags(write=False)
    return SimpleNamespace(B=B, R=Rn, C=C, dy=dy, y=y)


def check_spmm_result(c, got, act, yprev_on, zr, bf16, what):
    """got: logical [rows][B][C] fp32.  The bound over every element, then the exact parts bit for bit."""
    ref, bound = R.spmm_ref(c.rowptr, c.s, c.absum, act, c.yprev[act] if yprev_on else None, zr)
    if bf16:
        bound = bound + R.bf16_half_spacing(ref)
    check(got, ref, bound, what)
    assert R.is_plus_zero(got[c.empty]).all(), what + ": an empty row is not +0"
    if zr >= 0:
        assert R.is_plus_zero(got[zr]).all(), what + ": zero_row is not +0"
    if not yprev_on or act == 0:                                   # a row select copies its source
        for r in c.select:
            if r != zr:
                assert R.same_bits(got[r], c.x[c.col[c.rowptr[r]]]), what + ": row select %d is not a copy" % r


def spmm_sweep(rows, cols, B, C, bf16):
    """All six activation epilogues and no epilogue x zero_row in {-1, 13, rows - 1} x (x, y, yprev) each vertex- or batch-major.
    -> the profiler's records and the number of launches."""
    c = spmm_case(rows, cols, B, C, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    csr = csr_dev(c)
    xs = {l: put(c.x, l, dt) for l in LAYS}
    n = 0
    with profiled() as p:
        for act in (None,) + R.ACTS:
            yps = {l: put(c.yprev[act], l, dt) for l in LAYS} if act is not None else {None: None}
            for zr, xl, yl, ypl in itertools.product((-1, 13, rows - 1), LAYS, LAYS, yps):
                extra = 1 if yl == "vm" else 0                     # a vertex-major result has one more row: it must stay untouched
                y = blank(rows + extra, B, C, yl, dt)
                rc = k_spmm(bf16, csr, xs[xl], strides(xl, cols, B, C), y, strides(yl, rows + extra, B, C), yps[ypl],
                            strides(ypl, rows, B, C) if ypl else (0, 0), act or 0, zr, B, rows, C)
                what = "spmm%s rows=%d B=%d C=%d act=%s zero_row=%d x=%s y=%s yprev=%s" % ("_bf16" if bf16 else "", rows, B, C, act, zr, xl, yl, ypl)
                assert rc == 0, (what, rc, _lib.load().sh_last_error())
                got = get(y, yl)
                assert np.isnan(got[rows:]).all(), what + ": wrote past the last row"
                check_spmm_result(c, got[:rows], act or 0, act is not None, zr, bf16, what)
                n += 1
    return p.recs, n


# ------------------------------------------------------------------------------------------------------------ sh_spmm, fp32
# launcher's rule (sh_spmm_p3): the vector form when C % 4 == 0, every stride % 4 == 0 and x, y, yprev are 16-byte aligned; a work item
# is a 256-element (vector form: 256-quad) part of a row; the grid is min(items, 4096) workgroups that stride over the items.
@pytest.mark.parametrize("rows,B,C,vec", [
    (ROWS, 5, 32, True),           # 40 quads: one part
    (ROWS, 33, 32, True),          # 264 quads: two parts, the last one ragged
    (ROWS, 5, 3, False),           # scalar through C: one part
    (ROWS, 100, 3, False),         # 300 elements: two parts
    (ROWS, 5, 6, False),           # C % 4 == 2
    (4200, 1, 4, True),            # 4200 items > 4096 workgroups: the grid-stride loop wraps
])
def test_spmm_f32_against_float64(rows, B, C, vec):
    recs, n = spmm_sweep(rows, COLS, B, C, False)
    assert n == 3 * (4 + 6 * 8)                                   # 3 zero rows x (no epilogue: 4 layout pairs + 6 epilogues x 8 triples)
    want = ("spmm_kernel<%s>" % ("true" if vec else "false"), "rows=%d B=%d C=%d" % (rows, B, C))
    assert len(recs) == n and set(recs) == {want}, (want, set(recs))


@pytest.mark.parametrize("how", ["x_offset", "x_stride", "y_stride", "yprev_stride"])
def test_spmm_f32_drops_to_the_scalar_form_on_alignment_or_stride(how):
    """C = 4 would take the vector form; an x that starts one float into its buffer, or a batch stride of 5 on x, y or yprev (rows
    padded by one float that holds NaN and must be neither read nor written), must take the scalar one - and still be right."""
    rows, B, C = ROWS, 5, 4
    c = spmm_case(rows, COLS, B, C, False)
    csr = csr_dev(c)

    def padded(a):                                                 # logical [n][B][C] -> device [n][B][5], last column NaN
        t = torch.full(a.shape[:2] + (5,), NAN)
        t[:, :, :C] = torch.tensor(a)
        return t.to(dev())

    if how == "x_offset":
        buf = torch.full((c.x.size + 1,), NAN, device=dev())
        buf[1:] = torch.tensor(c.x).reshape(-1).to(dev())
        x, xs = buf[1:], (B * C, C)
        assert x.data_ptr() % 16 == 4
    elif how == "x_stride":
        x, xs = padded(c.x), (B * 5, 5)
    else:
        x, xs = put(c.x, "vm"), (B * C, C)
    with profiled() as p:
        for act, zr in itertools.product((None,) + R.ACTS, (-1, 13, rows - 1)):
            if how == "yprev_stride" and act is None:
                continue
            yp = None if act is None else (padded(c.yprev[act]) if how == "yprev_stride" else put(c.yprev[act], "vm"))
            yps = (0, 0) if act is None else ((B * 5, 5) if how == "yprev_stride" else (B * C, C))
            y = torch.full((rows + 1, B, 5 if how == "y_stride" else C), NAN, device=dev())
            ys = (B * 5, 5) if how == "y_stride" else (B * C, C)
            what = "spmm %s act=%s zero_row=%d" % (how, act, zr)
            assert k_spmm(False, csr, x, xs, y, ys, yp, yps, act or 0, zr, B, rows, C) == 0, what
            got = y.cpu().numpy()
            assert np.isnan(got[rows:]).all() and np.isnan(got[:, :, C:]).all(), what + ": wrote outside the rows"
            check_spmm_result(c, np.ascontiguousarray(got[:rows, :, :C]), act or 0, act is not None, zr, False, what)
    assert p.recs and set(p.recs) == {("spmm_kernel<false>", "rows=%d B=%d C=%d" % (rows, B, C))}, set(p.recs)


# ---------------------------------------------------------------------------------------------------------------- sh_spmm_p3
# launcher's rule: the eight-channel kernel (spmm_p3x8_kernel; tag x8=1) for C >= 128 or (C == 64 and B >= 256), else the quad form
# (spmm_kernel<true, true>; x8=0); both are recorded as "spmm_kernel<true, p3>".  256 eight-channel pieces are one part of a row.
P3_QUAD = [(16, 16), (48, 32), (32, 64), (16, 96)]
P3_X8 = [(16, 128),                # 256 pieces: exactly one part
         (32, 128),                # 512: two parts
         (16, 160),                # 320: a ragged last part
         (256, 64),                # C = 64 takes this form from B = 256 on (2048 pieces)
         (16, 256)]


@pytest.mark.parametrize("B,C,x8", [(b, ch, 0) for b, ch in P3_QUAD] + [(b, ch, 1) for b, ch in P3_X8])
def test_spmm_p3_rows_are_spmm_rows_and_the_image_is_their_image(B, C, x8):
    rows = ROWS
    assert has_image(C) and B % 16 == 0
    c = spmm_case(rows, COLS, B, C, False)
    csr = csr_dev(c)
    x = put(c.x, "vm")
    nimg = _lib.load().sh_p3_bytes(rows, B, C)
    for act, zr in ((None, -1), (None, 13), (2, -1), (2, 13)):
        yp = None if act is None else put(c.yprev[act], "vm")
        what = "spmm_p3 B=%d C=%d act=%s zero_row=%d" % (B, C, act, zr)
        y0 = blank(rows, B, C, "vm")
        assert k_spmm(False, csr, x, (B * C, C), y0, (B * C, C), yp, (B * C, C) if act else (0, 0), act or 0, zr, B, rows, C) == 0
        check_spmm_result(c, get(y0, "vm"), act or 0, act is not None, zr, False, what + " (sh_spmm)")
        want_img = to_p3(y0)
        y = blank(rows, B, C, "vm")
        img = torch.full((nimg,), 0xFF, dtype=torch.uint8, device=dev())
        img_only = torch.full((nimg,), 0xFF, dtype=torch.uint8, device=dev())
        with profiled() as p:
            assert k_spmm_p3(csr, x, y, img, yp, act or 0, zr, B, rows, C) == 0, what
            assert k_spmm_p3(csr, x, None, img_only, yp, act or 0, zr, B, rows, C) == 0, what
        assert p.recs == [("spmm_kernel<true, p3>", "rows=%d B=%d C=%d f32=%d x8=%d" % (rows, B, C, f, x8)) for f in (1, 0)], p.recs
        assert torch.equal(y.view(torch.int32), y0.view(torch.int32)), what + ": fp32 rows differ from sh_spmm's"
        assert torch.equal(img, want_img), what + ": image is not the image of the rows"
        assert torch.equal(img_only, want_img), what + ": image-only call differs"


@pytest.mark.parametrize("B,C", [(8, 32), (16, 24)])
def test_spmm_p3_refuses_shapes_without_an_image(B, C):
    rows = ROWS
    c = spmm_case(rows, COLS, B, C, False)
    y = blank(rows, B, C, "vm")
    img = torch.full((4096,), 0xFF, dtype=torch.uint8, device=dev())
    with profiled() as p:
        rc = k_spmm_p3(csr_dev(c), put(c.x, "vm"), y, img, None, 0, -1, B, rows, C)
    assert rc == SH_ERR_UNSUPPORTED and p.recs == []
    assert torch.isnan(y).all() and bool((img == 0xFF).all())


# -------------------------------------------------------------------------------------------------------------- sh_spmm_bf16
# launcher's rule: C % 8 == 0 and 16-byte aligned rows or SH_ERR_UNSUPPORTED; a work item is 256 eight-channel pieces of a row; the
# grid is min(items, 8192) workgroups that stride over the items.
@pytest.mark.parametrize("rows,B,C", [
    (ROWS, 5, 8), (ROWS, 5, 16), (ROWS, 5, 24), (ROWS, 5, 128),
    (ROWS, 33, 64),                # 264 pieces: two parts, the last one ragged
    (8300, 1, 8),                  # 8300 items > 8192 workgroups: the grid-stride loop wraps
])
def test_spmm_bf16_against_float64(rows, B, C):
    recs, n = spmm_sweep(rows, COLS, B, C, True)
    assert n == 3 * (4 + 6 * 8)
    assert len(recs) == n and set(recs) == {("spmm_bf16_kernel", "rows=%d B=%d C=%d" % (rows, B, C))}, set(recs)


@pytest.mark.parametrize("how", ["c12", "x_offset"])
def test_spmm_bf16_refuses_what_it_cannot_load_in_16_bytes(how):
    rows, B, C = ROWS, 5, 12 if how == "c12" else 8
    rng = np.random.default_rng(3)
    rowptr, col, val = R.make_csr(rows, COLS, 1)
    csr = tuple(torch.from_numpy(a).to(dev()) for a in (rowptr, col, val))
    buf = R.to_bf16(rng.standard_normal(COLS * B * C + 8)).to(dev())
    x = buf[1:] if how == "x_offset" else buf
    y = blank(rows, B, C, "vm", torch.bfloat16)
    with profiled() as p:
        rc = k_spmm(True, csr, x, (B * C, C), y, (B * C, C), None, (0, 0), 0, -1, B, rows, C)
    assert rc == SH_ERR_UNSUPPORTED and p.recs == []
    assert torch.isnan(y).all()


# ----------------------------------------------------------------------------------------------------------- sh_act_backward
def check_act_result(c, got, act, zr, bf16, what):
    ref, bound = R.act_backward_ref(c.dy, c.y[act], act, zr)
    if bf16:
        bound = bound + R.bf16_half_spacing(ref)
    check(got, ref, bound, what)
    if zr >= 0:
        assert R.is_plus_zero(got[zr]).all(), what + ": zero_row is not +0"
    if act in (0, 1):                                              # identity: dy; ReLU: dy or 0 - one exact fp32 product
        exact = c.dy * (np.ones_like(c.dy) if act == 0 else (c.y[act] > 0).astype(np.float32))
        if zr >= 0:
            exact[zr] = 0.0
        assert R.same_bits(got, exact), what + ": not bitwise dy / 0"


def act_sweep(B, Rn, C, bf16, lay_triples, zero_rows):
    """All six activations x zero rows x (dy, y, dpre) layouts; a vertex-major dpre has two more rows that must stay untouched."""
    c = act_case(B, Rn, C, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    dys = {l: put(c.dy, l, dt) for l in LAYS}
    for act in R.ACTS:
        ys = {l: put(c.y[act], l, dt) for l in LAYS}
        for zr, (dl, yl, pl) in itertools.product(zero_rows, lay_triples):
            extra = 2 if pl == "vm" else 0
            dp = blank(Rn + extra, B, C, pl, dt)
            what = "act_backward%s B=%d R=%d C=%d act=%d zero_row=%d dy=%s y=%s dpre=%s" % ("_bf16" if bf16 else "", B, Rn, C, act, zr, dl, yl, pl)
            rc = k_act(bf16, dys[dl], strides(dl, Rn, B, C), ys[yl], strides(yl, Rn, B, C), dp, strides(pl, Rn + extra, B, C), B, Rn, C, act, zr)
            assert rc == 0, (what, rc, _lib.load().sh_last_error())
            got = get(dp, pl)
            assert np.isnan(got[Rn:]).all(), what + ": wrote past the last row"
            check_act_result(c, got[:Rn], act, zr, bf16, what)


ALL_TRIPLES = list(itertools.product(LAYS, LAYS, LAYS))
# launcher's rule (sh_act_backward_tr_img): the TURN form when C <= 8, dy and y are the same batch-major layout (row stride C, equal batch
# strides >= R C), dpre is vertex-major contiguous and 16 (B C + 1) floats fit 64 KiB of LDS; else the VECTOR form when C % 4 == 0,
# every stride % 4 == 0 and all three tensors are 16-byte aligned; else the SCALAR form.  Vector / scalar: a work item is a 256-quad /
# 256-element part of a row, min(items, 8192) workgroups stride over the items.


@pytest.mark.parametrize("B,Rn,C", [
    (5, 19, 32),                   # vector: 40 quads, one part
    (33, 19, 32),                  # vector: 264 quads, two parts, the last one ragged
])
def test_act_backward_vector_form(B, Rn, C):
    act_sweep(B, Rn, C, False, ALL_TRIPLES, (-1, 13, Rn - 1))       # C = 32 > 8: never the turn form


def test_act_backward_scalar_form_through_the_channel_count():
    # C = 6: C % 4 != 0 -> scalar; the triple (bm, bm, vm) alone would be the turn form (C <= 8) and is left to the turn tests
    act_sweep(5, 19, 6, False, [t for t in ALL_TRIPLES if t != ("bm", "bm", "vm")], (-1, 13, 18))
    # C = 3, vertex-major in (row stride B C != C): scalar, two parts at B = 100 (300 elements)
    act_sweep(5, 19, 3, False, [("vm", "vm", "vm"), ("vm", "vm", "bm")], (-1, 13, 18))
    act_sweep(100, 19, 3, False, [("vm", "vm", "vm")], (-1, 18))


def test_act_backward_scalar_form_through_a_misaligned_dy():
    """C = 4, all vertex-major (B = 5: row stride 20 != C, so not the turn form): the vector form but for a dy that starts one float into
    its buffer."""
    B, Rn, C = 5, 19, 4
    c = act_case(B, Rn, C, False)
    buf = torch.full((c.dy.size + 1,), NAN, device=dev())
    buf[1:] = torch.tensor(c.dy).reshape(-1).to(dev())
    dy = buf[1:]
    assert dy.data_ptr() % 16 == 4
    for act, zr in itertools.product(R.ACTS, (-1, 13, Rn - 1)):
        dp = blank(Rn + 2, B, C, "vm")
        what = "act_backward misaligned dy act=%d zero_row=%d" % (act, zr)
        assert k_act(False, dy, (B * C, C), put(c.y[act], "vm"), (B * C, C), dp, (B * C, C), B, Rn, C, act, zr) == 0, what
        got = get(dp, "vm")
        assert np.isnan(got[Rn:]).all(), what
        check_act_result(c, got[:Rn], act, zr, False, what)


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("Rn", [1, 17, 19, 33])
def test_act_backward_turn_form(Rn, C):
    """Batch-major dy / y, vertex-major dpre, C <= 8: 16-row tiles turned in LDS.  R = 1: one partial tile; 17, 19, 33: full tiles and a
    last tile of 1, 3, 1 rows.  zero_row: none, the first row, the first row of the last tile, the last row."""
    zrs = sorted({-1, 0, (Rn - 1) // 16 * 16, Rn - 1})
    act_sweep(5, Rn, C, False, [("bm", "bm", "vm")], zrs)


@pytest.mark.parametrize("B", [341,       # turn: 16 (341 * 3 + 1) floats = 65536 bytes, exactly the bound
                               342])      # 16 (342 * 3 + 1) floats = 65728 bytes > 64 KiB: the general launcher, scalar form (C % 4 != 0)
def test_act_backward_at_and_past_the_lds_bound(B):
    act_sweep(B, 17, 3, False, [("bm", "bm", "vm")], (-1, 16))


def test_act_backward_turn_form_on_a_view_with_a_longer_batch_stride():
    """dy / y are the first R rows of batch-major [B][R + 3][C] buffers (batch stride (R + 3) C > R C); the other rows hold NaN."""
    B, Rn, C = 5, 19, 3
    c = act_case(B, Rn, C, False)

    def view(a):
        t = torch.full((B, Rn + 3, C), NAN)
        t[:, :Rn] = torch.tensor(a).permute(1, 0, 2)
        return t.to(dev())

    dy = view(c.dy)
    for act, zr in itertools.product(R.ACTS, (-1, 17, Rn - 1)):
        dp = blank(Rn + 2, B, C, "vm")
        what = "act_backward view act=%d zero_row=%d" % (act, zr)
        assert k_act(False, dy, (C, (Rn + 3) * C), view(c.y[act]), (C, (Rn + 3) * C), dp, (B * C, C), B, Rn, C, act, zr) == 0, what
        got = get(dp, "vm")
        assert np.isnan(got[Rn:]).all(), what
        check_act_result(c, got[:Rn], act, zr, False, what)


# -------------------------------------------------------------------------------------------------------- sh_act_backward_tr
RIDERS = [(9, 16, 32), (3, 3, 16)]                                 # (S, Cin, Cout): 4608 elements = 18 workgroups, 144 = 1 ragged one


@pytest.mark.parametrize("form", ["vector", "turn"])
def test_act_backward_riders_transpose_the_weights_and_leave_dpre_alone(form):
    if form == "vector":
        # R = 1, B = 1, C = 4: a single main workgroup in front of the riders'.  With one row and one batch entry every layout is the
        # same memory, and equal dy / y batch strides would make it the turn form: y's (never used: B = 1) is 8, which the turn rule refuses
        B, Rn, C, dys, ys = 1, 1, 4, (4, 4), (4, 8)
    else:
        B, Rn, C, dys, ys = 5, 17, 3, (3, 17 * 3), (3, 17 * 3)     # two main workgroups
    c = act_case(B, Rn, C, False)
    lay = "vm" if form == "vector" else "bm"
    act, zr = 2, -1 if form == "vector" else Rn - 1
    dy, y = put(c.dy, lay), put(c.y[act], lay)
    g = torch.Generator().manual_seed(11)
    ws = [torch.randn(co, s * ci, generator=g).to(dev()) for s, ci, co in RIDERS]
    want_t = [ops.weight_transpose(w, s, ci, co) for w, (s, ci, co) in zip(ws, RIDERS)]
    plain = blank(Rn + 2, B, C, "vm")
    assert k_act(False, dy, dys, y, ys, plain, (B * C, C), B, Rn, C, act, zr) == 0
    check_act_result(c, get(plain, "vm")[:Rn], act, zr, False, "act_backward (%s form, no riders)" % form)
    outs = [torch.full((ci, s * co), NAN, device=dev()) for s, ci, co in RIDERS]
    dp = blank(Rn + 2, B, C, "vm")
    assert k_act_tr(dy, dys, y, ys, dp, (B * C, C), B, Rn, C, act, zr, ws, outs, RIDERS) == 0
    assert torch.equal(dp[:Rn].view(torch.int32), plain[:Rn].view(torch.int32)) and torch.isnan(dp[Rn:]).all()
    for o, w in zip(outs, want_t):
        assert torch.equal(o.view(torch.int32), w.view(torch.int32))
    for (s, ci, co), w, o in zip(RIDERS, ws, outs):                # and the transpose is the definition: wt[ci][s Cout + co] = w[co][s Cin + ci]
        assert torch.equal(o.cpu(), w.cpu().view(co, s, ci).permute(2, 1, 0).reshape(ci, s * co))


def test_act_backward_riders_above_the_limit_are_an_error():
    B, Rn, C = 1, 1, 4
    c = act_case(B, Rn, C, False)
    n = 33                                                         # the launch carries at most 32 transposes
    ws = [torch.zeros(4, 4, device=dev()) for _ in range(n)]
    outs = [torch.full((4, 4), NAN, device=dev()) for _ in range(n)]
    dp = blank(Rn, B, C, "vm")
    rc = k_act_tr(put(c.dy, "vm"), (4, 4), put(c.y[2], "vm"), (4, 8), dp, (4, 4), B, Rn, C, 2, -1, ws, outs, [(1, 4, 4)] * n)
    assert rc == SH_ERR_INVALID_ARG
    assert torch.isnan(dp).all() and all(bool(torch.isnan(o).all()) for o in outs)
    assert k_act_tr(put(c.dy, "vm"), (4, 4), put(c.y[2], "vm"), (4, 8), dp, (4, 4), B, Rn, C, 2, -1, ws[:32], outs[:32], [(1, 4, 4)] * 32) == 0
    assert not torch.isnan(dp).any() and all(bool((o == 0).all()) for o in outs[:32]) and bool(torch.isnan(outs[32]).all())


# ---------------------------------------------------------------------------------------------------- sh_act_backward_tr_img
@pytest.mark.parametrize("B,C", [(16, 16), (48, 32), (16, 128)])
def test_act_backward_image_is_the_image_of_dpre(B, C):
    Rn = 19
    c = act_case(B, Rn, C, False)
    dy = put(c.dy, "vm")
    sv = (B * C, C)
    nimg = _lib.load().sh_p3_bytes(Rn, B, C)
    for act, zr in itertools.product(R.ACTS, (-1, Rn - 1)):
        y = put(c.y[act], "vm")
        dp = blank(Rn, B, C, "vm")
        img = torch.full((nimg,), 0xFF, dtype=torch.uint8, device=dev())
        what = "act_backward_tr_img B=%d C=%d act=%d zero_row=%d" % (B, C, act, zr)
        assert k_act_tr(dy, sv, y, sv, dp, sv, B, Rn, C, act, zr, [], [], [], img=img, with_img=True) == 0, what
        check_act_result(c, get(dp, "vm"), act, zr, False, what)
        assert torch.equal(img, to_p3(dp)), what + ": image is not the image of dpre"


@pytest.mark.parametrize("why,B,C,lay", [("batch not a multiple of 16", 8, 32, "vm"),
                                         ("turn form (batch-major in, C <= 8)", 16, 8, "bm")])
def test_act_backward_image_refusals(why, B, C, lay):
    Rn = 19
    c = act_case(B, Rn, C, False)
    dp = blank(Rn, B, C, "vm")
    img = torch.full((4096,), 0xFF, dtype=torch.uint8, device=dev())
    st = strides(lay, Rn, B, C)
    rc = k_act_tr(put(c.dy, lay), st, put(c.y[2], lay), st, dp, (B * C, C), B, Rn, C, 2, -1, [], [], [], img=img, with_img=True)
    assert rc == SH_ERR_UNSUPPORTED, why
    assert torch.isnan(dp).all() and bool((img == 0xFF).all())


# ------------------------------------------------------------------------------------------------------ sh_act_backward_bf16
@pytest.mark.parametrize("B,Rn,C", [
    (5, 19, 8), (5, 19, 24), (5, 19, 64),
    (33, 19, 64),                  # 264 pieces: two parts, the last one ragged
    (1, 8300, 8),                  # 8300 items > 8192 workgroups: the grid-stride loop wraps
])
def test_act_backward_bf16_against_float64(B, Rn, C):
    act_sweep(B, Rn, C, True, [("vm", "vm", "vm"), ("bm", "bm", "vm"), ("vm", "bm", "bm")], (-1, 13, Rn - 1))


@pytest.mark.parametrize("how", ["c12", "dy_offset"])
def test_act_backward_bf16_refuses_what_it_cannot_load_in_16_bytes(how):
    B, Rn, C = 5, 19, 12 if how == "c12" else 8
    rng = np.random.default_rng(4)
    buf = R.to_bf16(rng.standard_normal(Rn * B * C + 8)).to(dev())
    dy = buf[1:] if how == "dy_offset" else buf
    y = R.to_bf16(rng.standard_normal(Rn * B * C)).to(dev())
    dp = blank(Rn, B, C, "vm", torch.bfloat16)
    assert k_act(True, dy, (B * C, C), y, (B * C, C), dp, (B * C, C), B, Rn, C, 2, -1) == SH_ERR_UNSUPPORTED
    assert torch.isnan(dp).all()
