"""Float64 references, derived error bounds and input builders for the latent fully-connected kernels (csrc/linear.hip: sh_linear_fwd,
sh_linear_bwd_data, sh_linear_bwd_wgt, sh_linear_bwd_wgt_adam) and the multi-tensor optimiser (csrc/adam.hip, csrc/sh_adam.h:
sh_adam_step, sh_adam_step_bf16, sh_adam_bump).  Test infrastructure only; nothing here is on the product path.

References work on operands already rounded to the kernel's input type (fp32, or fp32 rounded to bf16), so the bounds below hold
the kernel's own arithmetic and nothing else.  u = 2^-24 is the fp32 unit roundoff, e = 2^-8 the bf16 one (8 significand bits).

Exact form (fp32 MFMA; skinny_gemm_kernel, the stream / dma / tile kernels, colsum_kernel)
    |got - ref| <= (R + C_SUM) u absum          R = reduction length, absum = sum_r |a_r b_r| (+ |bias|)
  Every kernel adds the R products of an output element to ONE fp32 accumulator per reduction range, in some order: a term passes
  through at most R additions, each with one rounding, which is the classical (1 + u)^R - 1 bound on sum |a_r b_r|.  C_SUM = 21
  counts what comes on top, per term:
     1   the product itself, should the matrix pipe round it before adding (an FMA would not);
     2   split_reduce_kernel, one of its 16 slab lanes: lane j adds slabs j, j + 16, ... in sequence - at most two additions while
         the reduction is split at most 32 ways (sum_bound() asserts that; the sweep's largest split is 17);
    16   the in-order sum of the 16 lane sums (`t += red[k]`, starting from 0);
     1   the bias add (`t + bias`, or the `v += bias` of the unsplit epilogues);
     1   the second-order term: (1 + u)^n - 1 <= n u (1 + n u) and n^2 u <= 1 for n <= 4096, so one more u covers it.
  A split reduction gives every term range <= R additions inside its slab, so R still covers the slabs.  The bias gradient is the same
  sum with b_r = 1: the tile kernel adds M / 4 quads per lane and then two shuffled halves, colsum_kernel is a chain of M.

bf16x3 forms (split3 / planes3; linear_fwd_x3_kernel, linear_fwd_wide_x3_kernel, linear_bwd_data_x3_kernel, linear_bwd_wgt_x3_kernel)
    |got - ref| <= (R + C_SUM) u (1 + e)^4 absum + X3_DROP u absum
  sh_split3 (csrc/sh_bf16.h) writes x = h + m + l with h = rne_bf16(x), m = rne_bf16(x - h), l = x - h - m exactly: |x - h| <= e |x|
  (one rounding to 8 bits), so |m| <= e |x| (a rounding never crosses the power of two above), and |l| = |(x - h) - m| <= e |x - h| <=
  e^2 |x|.  Of the nine products of (h + m + l)(h' + m' + l') the kernels keep hh', hm', mh', mm', hl', lh' and drop ml', lm', ll':
      |m l'| + |l m'| + |l l'| <= (2 e^3 + e^4) |x x'| = (2 + 2^-8) u |x x'|            X3_DROP = 2 + 2^-8
  The kept products are exact in fp32 (8 x 8 bits) and are added to the fp32 accumulator by v_mfma_f32_16x16x32_bf16; their absolute
  sum is at most (1 + e + e^2)^2 <= (1 + e)^4 times |x x'|, which scales the accumulation term.  That term keeps the exact form's
  count R: six instructions of 32 products per 32 reduction indices, modelled as at most one rounding of the accumulator per
  reduction index.  tests/test_linear_ref_host.py emulates the scheme in numpy fp32 with a rounding after EVERY kept product (six
  per index) on the sweep's own inputs and measures the largest ratio error / bound; it must stay below 1 (measured: the dropped
  products reach 0.25 of X3_DROP u absum at M = 1, where one product is the whole sum, and the whole error 0.06 of the bound).

Adam (adam_update of csrc/sh_adam.h, contraction off: every fp32 operation rounds once)
  adam64() evaluates the update in float64 from the fp32 inputs and the kernel's own fp32 coefficients, and carries for every
  intermediate an absolute error bound E(.): for z = fl(x op y), E(z) = (first-order propagation of E(x), E(y) through op) +
  u (|z| + that) + 2^-149, i.e. one rounding relative to the computed value and one subnormal step.  The operations, in order:
      g' = g + wd p                 (two, only when wd != 0)
      d  = g' - m
      m' = m + w d                  (w < 0.5)         or        g' - d (1 - w)        (w >= 0.5; 1 - w is exact there)
      v' = b2 v + (w2 g') g'        (four)
      den = sqrt(v') / bc2_sqrt + eps      (three; sqrtf and the division are correctly rounded in the default build)
      p' = p - step_size m' / den          (three)
  The square root propagates E(v') as the larger of sqrt(v') - sqrt(max(v' - E, 0)) and sqrt(v' + E) - sqrt(v'), a quotient x / y as
  (E(x) + |x / y| E(y)) / (|y| - E(y)).  The bf16 shadow is not compared with float64: it is rne_bf16 of the kernel's OWN new weight,
  bit for bit.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
E_BF16 = 2.0 ** -8
C_SUM = 21
X3_DROP = 2.0 + 2.0 ** -8
TINY = 2.0 ** -149
MAX_SPLIT = 32


# ------------------------------------------------------------------------------------------------------------------- builders
def to_bf16(a):
    """fp32 / float64 numpy -> the values rounded to bf16 (round to nearest even), as a torch.bfloat16 CPU tensor."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def bf16_round(a):
    """fp32 numpy -> fp32 numpy holding the values rounded to bf16 (round to nearest even)."""
    return to_bf16(a).float().numpy()


def bf16_bits(a):
    """fp32 numpy -> uint16 bit patterns of rne_bf16(a), in integer arithmetic (independent of torch's cast)."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return r.astype(np.uint16)


def seed_of(M, N, K):
    """The seed of a shape's operands in the GPU sweep (and in the host checks made on the sweep's own inputs)."""
    return 1000003 * M + 1009 * N + K


def operands(M, N, K, seed, bf16=False):
    """Standard normal x [M][K], dy [M][N], bias [N] and W [N][K] / sqrt(K), fp32 (rounded to bf16 when asked), fixed seed."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32)
    b = rng.standard_normal((N,)).astype(np.float32)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    if bf16:
        x, w, b, dy = bf16_round(x), bf16_round(w), b, bf16_round(dy)
    return x, w, b, dy


# ----------------------------------------------------------------------------------------------------------------- references
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def fwd64(x, w, bias=None):
    """y = x W^T + b -> (y, absum) float64 [M][N]; absum = sum_k |x W| + |b|."""
    x, w = _f64(x), _f64(w)
    y, ab = x @ w.T, np.abs(x) @ np.abs(w).T
    if bias is not None:
        y, ab = y + _f64(bias)[None, :], ab + np.abs(_f64(bias))[None, :]
    return y, ab


def bwd_data64(dy, w):
    """dx = dy W -> (dx, absum) float64 [M][K]."""
    dy, w = _f64(dy), _f64(w)
    return dy @ w, np.abs(dy) @ np.abs(w)


def bwd_wgt64(dy, x):
    """dW = dy^T x, db = sum_m dy -> (dW, absum_W [N][K], db, absum_b [N])."""
    dy, x = _f64(dy), _f64(x)
    return dy.T @ x, np.abs(dy).T @ np.abs(x), dy.sum(axis=0), np.abs(dy).sum(axis=0)


def sum_bound(absum, R, x3=False, split=1):
    """Per-element bound of a product sum of reduction length R (module docstring).  x3: a bf16x3 kernel ran."""
    assert 1 <= split <= MAX_SPLIT, "C_SUM counts two additions per slab lane: split <= 32"
    assert R + C_SUM <= 4096, "the second-order term of C_SUM needs n <= 4096"
    if not x3:
        return (R + C_SUM) * U * absum
    return ((R + C_SUM) * (1.0 + E_BF16) ** 4 + X3_DROP) * U * absum


# ------------------------------------------------------------------------------------------------- bf16x3 emulation (host check)
def split3(a):
    """fp32 numpy -> (h, m, l) fp32 numpy, sh_split3's three terms: h = rne_bf16(a), m = rne_bf16(a - h), l = a - h - m."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    h = bf16_round(a)
    r = (a - h).astype(np.float32)
    m = bf16_round(r)
    l = (r - m).astype(np.float32)
    return h, m, l


def x3_emulate(a, b):
    """sum_r a[i][r] b[j][r] in the six-of-nine scheme, fp32 accumulation with a rounding after every kept product, in lin_x3_mma's
    order (l h', h l', m m', m h', h m', h h') per block of 32 reduction indices.  a [I][R], b [J][R] fp32 -> fp32 [I][J]."""
    ah, am, al = split3(a)
    bh, bm, bl = split3(b)
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    R = a.shape[1]
    for r0 in range(0, R, 32):
        for p, q in ((al, bh), (ah, bl), (am, bm), (am, bh), (ah, bm), (ah, bh)):
            for r in range(r0, min(R, r0 + 32)):
                prod = (p[:, r:r + 1].astype(np.float32) * q[None, :, r]).astype(np.float32)        # exact: 8 x 8 bits
                acc = (acc + prod).astype(np.float32)
    return acc


def x3_dropped(a, b):
    """The dropped part of the same sum in float64: sum_r (m l' + l m' + l l')."""
    ah, am, al = (_f64(t) for t in split3(a))
    bh, bm, bl = (_f64(t) for t in split3(b))
    return am @ bl.T + al @ bm.T + al @ bl.T


# ------------------------------------------------------------------------------------------------------------------------ Adam
def pow_int(b, n):
    """sh_pow_int: b^n by repeated squaring in double, the same operations in the same order."""
    r = 1.0
    n = int(n)
    while n:
        if n & 1:
            r *= b
        b *= b
        n >>= 1
    return r


def adam_coeffs(beta1, beta2, steps_done, lr):
    """sh_adam_coeffs -> (step_size, bc2_sqrt) as the fp32 values the kernel holds.  lr: the fp32 device scalar's value."""
    step = int(np.float32(steps_done)) + 1
    bc1 = 1.0 - pow_int(float(beta1), step)
    bc2 = 1.0 - pow_int(float(beta2), step)
    return np.float32(float(np.float32(lr)) / bc1), np.float32(math.sqrt(bc2))


def adam_hyper(beta1, beta2, eps, wd):
    """The kernel's fp32 coefficients (w1, b2, w2, eps, wd) from the double hyper-parameters."""
    return (np.float32(1.0 - beta1), np.float32(beta2), np.float32(1.0 - beta2), np.float32(eps), np.float32(wd))


class _V:
    """A float64 value with an absolute bound on the error of its fp32-computed counterpart."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = _f64(v)
        self.e = np.zeros_like(self.v) if e is None else e

    def _rounded(self, v, e):
        return _V(v, e + U * (np.abs(v) + e) + TINY)

    def add(self, o, sign=1.0):
        return self._rounded(self.v + sign * o.v, self.e + o.e)

    def sub(self, o):
        return self.add(o, -1.0)

    def mul(self, o):
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def div(self, o):
        q = self.v / o.v
        return self._rounded(q, (self.e + np.abs(q) * o.e) / (np.abs(o.v) - o.e))

    def sqrt(self):
        s = np.sqrt(self.v)
        return self._rounded(s, np.maximum(s - np.sqrt(np.maximum(self.v - self.e, 0.0)), np.sqrt(self.v + self.e) - s))


def adam64(p, g, m, v, steps_done, lr, beta1, beta2, eps, wd):
    """torch.optim.Adam's update (coupled weight decay) as csrc/sh_adam.h computes it, in float64 from fp32 inputs.
    -> dict of (reference, bound) pairs for 'p', 'm', 'v' (float64 numpy, the inputs' shape)."""
    w1, b2, w2, epsf, wdf = adam_hyper(beta1, beta2, eps, wd)
    step_size, bc2_sqrt = adam_coeffs(beta1, beta2, steps_done, lr)
    c = lambda s: _V(np.float64(s))                                    # noqa: E731 - an exact fp32 constant
    P, G, M, Vv = _V(p), _V(g), _V(m), _V(v)
    if wdf != 0:
        G = G.add(c(wdf).mul(P))
    d = G.sub(M)
    if w1 < np.float32(0.5):
        Mn = M.add(c(w1).mul(d))
    else:
        one_w = np.float32(1.0) - w1                                   # exact for w in [0.5, 1]
        assert float(one_w) == 1.0 - float(w1)
        Mn = G.sub(d.mul(c(one_w)))
    Vn = c(b2).mul(Vv).add(c(w2).mul(G).mul(G))
    den = Vn.sqrt().div(c(bc2_sqrt)).add(c(epsf))
    Pn = P.sub(c(step_size).mul(Mn).div(den))
    return {"p": (Pn.v, Pn.e), "m": (Mn.v, Mn.e), "v": (Vn.v, Vn.e)}


def adam_f32(p, g, m, v, steps_done, lr, beta1, beta2, eps, wd):
    """adam_update transcribed in numpy fp32, operation by operation (no contraction) -> (p, m, v) fp32."""
    f = np.float32
    w1, b2, w2, epsf, wdf = adam_hyper(beta1, beta2, eps, wd)
    step_size, bc2_sqrt = adam_coeffs(beta1, beta2, steps_done, lr)
    p, g, m, v = (np.ascontiguousarray(t, dtype=f) for t in (p, g, m, v))
    if wdf != 0:
        g = (g + (wdf * p).astype(f)).astype(f)
    d = (g - m).astype(f)
    if w1 < f(0.5):
        m = (m + (w1 * d).astype(f)).astype(f)
    else:
        m = (g - (d * (f(1.0) - w1)).astype(f)).astype(f)
    v = ((b2 * v).astype(f) + ((w2 * g).astype(f) * g).astype(f)).astype(f)
    den = ((np.sqrt(v).astype(f) / bc2_sqrt).astype(f) + epsf).astype(f)
    p = (p - ((step_size * m).astype(f) / den).astype(f)).astype(f)
    return p, m, v


def adam_state(n, seed, steps_done, zero_grad_at=()):
    """fp32 (p, g, m, v) of n elements: standard normal p and g, moments zero before the first step and plausible after it
    (m ~ 0.1 N(0, 1), v = (0.1 N(0, 1))^2); exact zeros in g, with v = 0 there, at the given indices."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    if steps_done > 0:
        m = (0.1 * rng.standard_normal(n)).astype(np.float32)
        v = ((0.1 * rng.standard_normal(n)) ** 2).astype(np.float32)
    else:
        m, v = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    for i in zero_grad_at:
        if i < n:
            g[i], v[i] = 0.0, 0.0
    return p, g, m, v


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    k = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool((a.view(k) == b.view(k)).all())
