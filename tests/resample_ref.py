"""Float64 references, derived error bounds and input builders for the re-sampling kernels (csrc/spmm_loss.hip: sh_spmm, sh_spmm_p3;
csrc/bf16_misc.hip: sh_spmm_bf16) and the activation-backward kernels (csrc/spiral_conv.hip: sh_act_backward, _tr, _tr_img;
csrc/bf16_misc.hip: sh_act_backward_bf16).  Test infrastructure only; nothing here is on the product path.

Every array here is LOGICAL vertex-major, [rows][B][C]; tests/test_resample_act.py lays it out for the kernel (batch-major,
vertex-major, views).  References work on operands already rounded to the kernel's input type, so the bounds below hold the kernel's
own arithmetic and nothing else.

Bounds (u = 2^-24, the fp32 unit roundoff; none is measured):

  fp32 spmm          |got - ref| <= (nnz_r + 4) u absum max(|act'|, 1) + u |s|
                     a chain of nnz_r fp32 FMAs rounds once per entry (absum = sum_e |val_e x_e|); the derivative is at most three
                     more roundings relative to the product (two inside act', one for the product); the additive term is the
                     absolute error of 1 - y^2 / y (1 - y) / y + 1 near their cancellation, times the sum s it multiplies.
  fp32 act backward  |got - ref| <= |dy| (4 u |act'(y)| + u)        the same two terms for a single product
  bf16 outputs       half the bf16 spacing at |ref| (one round-to-nearest: 2^-8 2^floor(log2 |ref|)) plus the fp32 bound above
"""
import numpy as np
import torch

from tests.p3_ref import ACT64, DACT64

U = 2.0 ** -24
LEAKY = float(np.float32(0.02))            # the constant the kernels hold (0.02f), not the double 0.02
ACTS = (0, 1, 2, 3, 4, 5)                  # identity, relu, elu, leaky_relu, sigmoid, tanh (enum sh_act)
COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9)       # entries per row, cycled: an empty row, every remainder of the 4- and 2-entry unrolls,
#                                            two trips of the 4-entry loop


def make_csr(rows, cols, seed):
    """-> (rowptr int32 [rows + 1], col int32, val fp32).  Row r has COUNTS[r % 9] entries; columns are random with repeats, values
    N(0, 1); the single-entry row 1 (and every other single-entry row after it) is a row select: one entry of value exactly 1.0."""
    rng = np.random.default_rng(seed)
    cnt = np.array([COUNTS[r % len(COUNTS)] for r in range(rows)], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    col = rng.integers(0, cols, size=int(rowptr[-1])).astype(np.int32)
    val = rng.standard_normal(int(rowptr[-1])).astype(np.float32)
    singles = np.flatnonzero(cnt == 1)
    val[rowptr[singles[::2]]] = 1.0
    return rowptr, col, val


def row_counts(rowptr):
    return np.diff(rowptr.astype(np.int64))


def select_rows(rowptr, val):
    """Rows that are a single entry of value exactly 1.0."""
    cnt = row_counts(rowptr)
    return np.array([r for r in np.flatnonzero(cnt == 1) if val[rowptr[r]] == 1.0], dtype=np.int64)


def dense(rowptr, col, val, cols):
    """The matrix as a float64 array (repeated columns add up)."""
    rows = len(rowptr) - 1
    m = np.zeros((rows, cols))
    for r in range(rows):
        for e in range(rowptr[r], rowptr[r + 1]):
            m[r, col[e]] += float(val[e])
    return m


def spmm64(rowptr, col, val, x):
    """x: [cols][B][C] (any float dtype, taken as the kernel's already rounded input) -> (y, absum), float64 [rows][B][C]:
    y[r] = sum_e val[e] x[col[e]], absum[r] = sum_e |val[e] x[col[e]]|.  A plain loop over rows and entries."""
    x = np.asarray(x, dtype=np.float64)
    rows = len(rowptr) - 1
    y = np.zeros((rows,) + x.shape[1:])
    absum = np.zeros_like(y)
    for r in range(rows):
        for e in range(int(rowptr[r]), int(rowptr[r + 1])):
            t = float(val[e]) * x[int(col[e])]
            y[r] += t
            absum[r] += np.abs(t)
    return y, absum


def act64(act, pre):
    """Activation in float64 (numpy in, numpy out)."""
    return ACT64[act](torch.from_numpy(np.ascontiguousarray(pre, dtype=np.float64))).numpy()


def dact64(act, y):
    """The activation's derivative taken from its OUTPUT y, float64, as the kernels take it (sh_act_grad_from_out)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    if act == 3:
        return np.where(y > 0, 1.0, LEAKY)
    return DACT64[act](torch.from_numpy(y)).numpy()


def to_bf16(a):
    """fp32 / float64 numpy -> the values rounded to bf16 (round to nearest even), as a torch.bfloat16 CPU tensor."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def bf16_np(t):
    """torch.bfloat16 tensor -> its exact values as float64 numpy."""
    return t.detach().float().cpu().numpy().astype(np.float64)


def act_output(act, shape, rng, bf16=False):
    """An activation OUTPUT of O(1) pre-activations, rounded to the kernel's input type (fp32, or fp32 rounded to bf16): it lies in
    the activation's range, as the tensor a backward pass is handed does.  -> fp32 numpy."""
    y = act64(act, rng.standard_normal(shape)).astype(np.float32)
    return to_bf16(y).float().numpy() if bf16 else y


def normal(shape, rng, bf16=False):
    a = rng.standard_normal(shape).astype(np.float32)
    return to_bf16(a).float().numpy() if bf16 else a


def spmm_ref(rowptr, s, absum, act=0, yprev=None, zero_row=-1):
    """Reference and bound of one sh_spmm call from spmm64's (s, absum): (ref, bound), float64 [rows][B][C]."""
    nnz = row_counts(rowptr).astype(np.float64)[:, None, None]
    if yprev is None:
        ref, bound = s.copy(), (nnz + 4) * U * absum
    else:
        d = dact64(act, yprev)
        ref = s * d
        bound = (nnz + 4) * U * absum * np.maximum(np.abs(d), 1.0) + U * np.abs(s)
    if zero_row >= 0:
        ref[zero_row] = 0.0
        bound[zero_row] = 0.0
    return ref, bound


def act_backward_ref(dy, y, act, zero_row=-1):
    """dpre = dy act'(y) with row zero_row forced to 0: (ref, bound), float64, from the rounded inputs dy and y."""
    dy = np.asarray(dy, dtype=np.float64)
    d = dact64(act, y)
    ref = dy * d
    bound = np.abs(dy) * (4 * U * np.abs(d) + U)
    if zero_row >= 0:
        ref[zero_row] = 0.0
        bound[zero_row] = 0.0
    return ref, bound


def bf16_half_spacing(ref):
    """Half the bf16 spacing at |ref| (8 significand bits): 2^-8 2^floor(log2 |ref|); 0 at 0."""
    m, e = np.frexp(np.abs(ref))                 # |ref| = m 2^e, m in [0.5, 1): floor(log2 |ref|) = e - 1
    return np.where(m > 0, np.ldexp(1.0, e - 1 - 8), 0.0)


def is_plus_zero(a):
    """Elementwise: the fp32 bit pattern is +0."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) == 0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
