"""Helpers of the three-plane tests (csrc/p3_conv.hip, csrc/wgrad_p3.hip): plane images (sh_to_p3 and a host decoder), three-plane
weight fragments, test operands and float64 activations.  Test infrastructure only; nothing here is on the product path."""
import ctypes

import numpy as np
import torch

from semantichuman_amd import _lib

SH_OK, SH_ERR_UNSUPPORTED = 0, -2

# float64 activations (reference models.py:19-32) and their derivatives expressed through the activation OUTPUT, as the kernels
# take them (sh_act_grad_from_out)
ACT64 = {0: lambda v: v, 1: torch.relu, 2: lambda v: torch.where(v > 0, v, torch.expm1(torch.clamp(v, max=0))),
         3: lambda v: torch.where(v > 0, v, 0.02 * v), 4: torch.sigmoid, 5: torch.tanh}
DACT64 = {0: lambda y: torch.ones_like(y), 1: lambda y: (y > 0).to(y.dtype), 2: lambda y: torch.where(y > 0, torch.ones_like(y), y + 1),
          3: lambda y: torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.02)), 4: lambda y: y * (1 - y), 5: lambda y: 1 - y * y}


def arr(vals, ct):
    return (ct * len(vals))(*vals)


def has_image(C):
    return C == 16 or (C > 0 and C % 32 == 0)


def wfrag3(w, S, cin, cout, tr):
    """Three-plane weight fragments of w [cout][S*cin]: the forward operand (tr False) or the backward-data one (tr True)."""
    lib = _lib.load()
    nb = lib.sh_conv_wfrag3_bytes(S, cout if tr else cin, cin if tr else cout)
    buf = torch.empty(nb, dtype=torch.uint8, device=w.device)
    _lib.check(lib.sh_conv_wfrag3_prep_multi(1, arr([w.data_ptr()], ctypes.c_void_p), arr([buf.data_ptr()], ctypes.c_void_p),
                                             arr([S], ctypes.c_int), arr([cin], ctypes.c_int), arr([cout], ctypes.c_int),
                                             arr([1 if tr else 0], ctypes.c_int), _lib.stream_ptr()), "wfrag3")
    return buf


def to_p3(x, rows=None):
    """x: [rows][B][C] vertex-major contiguous fp32 -> its plane image (uint8 tensor).  rows > x.shape[0]: the image buffer has
    room for that many rows and only the first x.shape[0] are written (the rest is left for the caller to fill)."""
    lib = _lib.load()
    n, B, C = x.shape
    nb = lib.sh_p3_bytes(rows or n, B, C)
    assert nb > 0, (n, B, C)
    buf = torch.empty(nb, dtype=torch.uint8, device=x.device)
    _lib.check(lib.sh_to_p3(_lib.ptr(x), B * C, C, _lib.ptr(buf), B, n, C, _lib.stream_ptr()), "sh_to_p3")
    return buf


def decode_image(img, rows, B, C):
    """Plane image (layout of include/sh_kernels.h / csrc/p3_conv.hip) -> the fp32 tensor [rows][B][C] it encodes, h + m + l
    evaluated in fp32 (exact: 8 + 8 + 8 significand bits)."""
    raw = img.cpu().numpy().view(np.uint16)
    nbg = B // 16
    if C == 16:
        a = raw.reshape(rows, nbg, 3, 2, 16, 8)                       # [row][bg][plane][kb2][b][8 ch]
        a = a.transpose(2, 0, 1, 4, 3, 5).reshape(3, rows, nbg * 16, 16)
    else:
        a = raw.reshape(rows, nbg, C // 32, 3, 4, 16, 8)              # [row][bg][cg][plane][kb][b][8 ch]
        a = a.transpose(3, 0, 1, 5, 2, 4, 6).reshape(3, rows, nbg * 16, C)
    f = (a.astype(np.uint32) << 16).view(np.float32)
    return torch.from_numpy(np.ascontiguousarray((f[0] + f[1]) + f[2]))


def _alt(n, period, dev):
    """+1 / -1 along an axis of length n: period 2 = + - + -, period 4 = + + - -."""
    return torch.where((torch.arange(n, device=dev) // (period // 2)) % 2 == 0, 1.0, -1.0)


def rnd(shape, dev, adversarial, gen, last=2, batch=0):
    """Training-scale operands (standard normal), or adversarial ones: magnitudes 10^U(-3,3) - six decades - with signs alternating
    along the last axis with period `last` and, for a batch > 0, along the batch axis (the second last) with that period.  The caller
    picks periods that differ between the two factors of a product, so the sums of every entry point cancel: forward and backward-data
    sum over channels (x and dpre alternate with period 2 along them, the weights with period 4 along theirs), the weight gradient
    over batch entries (x with period 2, dpre with period 4)."""
    x = torch.randn(shape, device=dev, generator=gen)
    if adversarial:
        mag = torch.pow(10.0, 6.0 * torch.rand(shape, device=dev, generator=gen) - 3.0)
        sgn = _alt(shape[-1], last, dev)
        if batch:
            sgn = sgn * _alt(shape[-2], batch, dev)[:, None]
        x = mag * sgn * (1.0 + 1e-3 * x)
    return x.float().contiguous()


def act_slope64(act, pre, e):
    """The largest slope of activation `act` over [pre - e, pre + e], elementwise (float64): by the mean value theorem an error of at
    most e in a pre-activation changes the activated value by at most that much times e."""
    if act == 0:
        return torch.ones_like(pre)
    hi = pre + e
    if act == 1:
        return (hi > 0).to(pre.dtype)
    if act == 2:
        return torch.exp(torch.clamp(hi, max=0))
    if act == 3:
        return torch.where(hi > 0, torch.ones_like(pre), torch.full_like(pre, 0.02))
    c = torch.sign(pre) * torch.clamp(pre.abs() - e, min=0)          # the point of the interval nearest 0, where these two are steepest
    if act == 4:
        sc = torch.sigmoid(c)
        return sc * (1 - sc)
    return 1 - torch.tanh(c) ** 2


def local_table(rng, R, n_in, S, none_frac=0.15):
    """A spiral-like gather table [R][S] over n_in input rows whose last row is the dummy: row r reads rows near r * (n_in - 1) / R
    (neighbouring rows share most of their sources, as on a mesh), about `none_frac` of the entries past the first are "no source"
    and point at the dummy row."""
    real = max(n_in - 1, 1)
    base = (np.arange(R, dtype=np.int64) * real) // max(R, 1)
    t = (base[:, None] + rng.integers(-5, 6, size=(R, S))) % real
    t[:, 0] = base
    none = rng.random((R, S)) < none_frac
    none[:, 0] = False
    t[none] = n_in - 1
    return np.ascontiguousarray(t.astype(np.int32))
