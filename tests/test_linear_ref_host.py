"""CPU checks of tests/linear_ref.py, the float64 references and bounds under tests/test_linear_edges.py: a reference or a bound that
is wrong would pass or fail the kernels for the wrong reason."""
import itertools

import numpy as np
import pytest
import torch

from tests import linear_ref as L

# the (M, N, K) at which the GPU sweep runs a bf16x3 kernel: forward (reduction K), backward-data (reduction N), weight gradient
# (reduction M)
X3_FWD = [(1, 256, 64), (33, 256, 64), (5, 256, 1056), (64, 256, 1088), (65, 256, 416), (65, 64, 32), (130, 128, 384), (200, 64, 352)]
X3_BWD = [(17, 96, 64), (64, 96, 64), (5, 1024, 64), (33, 1056, 256)]
X3_WGT = [(1, 64, 64), (17, 64, 320), (33, 192, 64), (64, 128, 256), (64, 64, 576)]


@pytest.mark.parametrize("M,N,K", [(5, 7, 13), (17, 64, 48), (3, 5, 2050)])
def test_references_are_the_float64_autograd_of_linear(M, N, K):
    x, w, b, dy = L.operands(M, N, K, seed=M + N + K)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tw = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    tb = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    ty = torch.nn.functional.linear(tx, tw, tb)
    ty.backward(torch.tensor(dy, dtype=torch.float64))
    y, ab = L.fwd64(x, w, b)
    assert np.abs(y - ty.detach().numpy()).max() <= 1e-12
    assert (np.abs(y) <= ab + 1e-12).all()
    y0, ab0 = L.fwd64(x, w, None)
    assert np.abs(y0 + b.astype(np.float64)[None] - y).max() <= 1e-12 and np.abs(ab0 + np.abs(b.astype(np.float64))[None] - ab).max() <= 1e-12
    dx, abx = L.bwd_data64(dy, w)
    assert np.abs(dx - tx.grad.numpy()).max() <= 1e-12 and (np.abs(dx) <= abx + 1e-12).all()
    dW, abw, db, abb = L.bwd_wgt64(dy, x)
    assert np.abs(dW - tw.grad.numpy()).max() <= 1e-12 and (np.abs(dW) <= abw + 1e-12).all()
    assert np.abs(db - tb.grad.numpy()).max() <= 1e-12 and (np.abs(db) <= abb + 1e-12).all()
    # absum is the sum of the absolute terms, element by element
    i, j = M - 1, N - 1
    assert abs(ab[i, j] - (np.abs(x[i].astype(np.float64) * w[j].astype(np.float64)).sum() + abs(float(b[j])))) <= 1e-12


def test_operands_are_fixed_and_scaled():
    x, w, b, dy = L.operands(17, 64, 320, seed=3)
    x2, w2, _, _ = L.operands(17, 64, 320, seed=3)
    assert np.array_equal(x, x2) and np.array_equal(w, w2)
    assert x.dtype == w.dtype == b.dtype == dy.dtype == np.float32
    assert 0.8 < x.std() < 1.2 and 0.8 < w.std() * np.sqrt(320) < 1.2
    xb, wb, _, dyb = L.operands(17, 64, 320, seed=3, bf16=True)
    for t in (xb, wb, dyb):
        assert np.array_equal(L.bf16_round(t), t)                        # already bf16 values
    assert not np.array_equal(xb, x)


def test_bf16_rounding_is_nearest_even_in_integer_arithmetic_too():
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(1 << 14) * np.exp(rng.uniform(-20, 20, 1 << 14))).astype(np.float32)
    a[:4] = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 0.0, -0.0], dtype=np.float32)       # two ties, the zeros
    via_torch = L.to_bf16(a).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(L.bf16_bits(a), via_torch)
    assert L.bf16_round(a[:2]).tolist() == [1.0, 1.0 + 2.0 ** -6]            # ties go to the even neighbour


def test_split3_is_exact_and_its_terms_are_as_small_as_the_derivation_says():
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(1 << 14) * np.exp(rng.uniform(-8, 8, 1 << 14))).astype(np.float32)
    h, m, l = L.split3(a)
    a64 = a.astype(np.float64)
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), a64)
    for t in (h, m, l):
        assert np.array_equal(L.bf16_round(t), t)                        # each term is a bf16 value
    assert (np.abs(a64 - h) <= L.E_BF16 * np.abs(a64)).all()
    assert (np.abs(m) <= L.E_BF16 * np.abs(a64)).all()
    assert (np.abs(l) <= L.E_BF16 ** 2 * np.abs(a64)).all()


def _x3_operands(kind, M, N, K):
    x, w, b, dy = L.operands(M, N, K, seed=L.seed_of(M, N, K))
    if kind == "fwd":
        return x, w, K                                                   # y[m][n] = sum_k x[m][k] w[n][k]
    if kind == "bwd":
        return dy, np.ascontiguousarray(w.T), N                          # dx[m][k] = sum_n dy[m][n] w^T[k][n]
    return np.ascontiguousarray(dy.T), np.ascontiguousarray(x.T), M      # dW[n][k] = sum_m dy^T[n][m] x^T[k][m]


@pytest.mark.parametrize("kind,shape", [("fwd", s) for s in X3_FWD] + [("bwd", s) for s in X3_BWD] + [("wgt", s) for s in X3_WGT])
def test_six_of_nine_emulation_stays_inside_the_split_bound(kind, shape):
    """numpy fp32: split both operands into three bf16 terms, keep six products, accumulate in fp32 with a rounding after every
    product.  Measured on these shapes: the dropped products reach at most 0.25 of X3_DROP u absum (at M = 1, where one product is the
    whole sum; the terms are rarely all at their worst), the whole error at most 0.06 of the bound."""
    a, b, R = _x3_operands(kind, *shape)
    a, b = a[:16], b[:48]                                               # a corner of the output: every reduction index, fewer elements
    ref = a.astype(np.float64) @ b.astype(np.float64).T
    absum = np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64)).T
    dropped = L.x3_dropped(a, b)
    ratio_d = float((np.abs(dropped) / (L.X3_DROP * L.U * absum)).max())
    got = L.x3_emulate(a, b)
    # kept + dropped is the exact product sum: the emulation's error against (ref - dropped) is accumulation alone
    bound = L.sum_bound(absum, R, x3=True)
    ratio = float((np.abs(got.astype(np.float64) - ref) / bound).max())
    print("x3 %s %s: dropped / (X3_DROP u absum) = %.4f, error / bound = %.4f" % (kind, shape, ratio_d, ratio))
    assert ratio_d <= 1.0 and ratio <= 1.0
    assert (np.abs(got.astype(np.float64) - (ref - dropped)) <= (R + L.C_SUM) * (1 + L.E_BF16) ** 4 * L.U * absum).all()
    assert not (np.abs(got.astype(np.float64) - ref) <= 0).all()        # and it is not vacuous: the emulation is not exact


def test_exact_bound_holds_a_sequential_fp32_sum_and_is_not_loose_by_orders():
    x, w, b, _ = L.operands(5, 64, 1040, seed=11)
    ref, absum = L.fwd64(x, w, b)
    acc = np.zeros((5, 64), dtype=np.float32)
    for k in range(1040):
        acc = (acc + (x[:, k:k + 1] * w[None, :, k]).astype(np.float32)).astype(np.float32)
    acc = (acc + b[None]).astype(np.float32)
    bound = L.sum_bound(absum, 1040, split=17)
    err = np.abs(acc.astype(np.float64) - ref)
    assert (err <= bound).all()
    # dropping the last 16 of 1040 products must break it: that is the mistake the bound exists to see
    short, _ = L.fwd64(x[:, :1024], w[:, :1024], b)
    assert (np.abs(short - ref) > bound).mean() > 0.5
    with pytest.raises(AssertionError):
        L.sum_bound(absum, 1040, split=33)


HYPER = list(itertools.product([(0.9, 0.999), (0.5, 0.999), (0.0, 0.5)], [0.0, 5e-5], [0, 1, 7, 999]))


@pytest.mark.parametrize("betas,wd,step", HYPER)
def test_fp32_transcription_of_adam_update_stays_inside_the_adam_bound(betas, wd, step):
    p, g, m, v = L.adam_state(8197, seed=step + 1, steps_done=step, zero_grad_at=(0, 5, 4096, 8196))
    lr = np.float32(1e-3)
    ref = L.adam64(p, g, m, v, step, lr, betas[0], betas[1], 1e-8, wd)
    got = dict(zip("pmv", L.adam_f32(p, g, m, v, step, lr, betas[0], betas[1], 1e-8, wd)))
    for k in "pmv":
        r, bnd = ref[k]
        err = np.abs(got[k].astype(np.float64) - r)
        assert np.isfinite(got[k]).all() and np.isfinite(r).all() and np.isfinite(bnd).all(), k
        assert (err <= bnd).all(), "%s: worst error / bound %.3f" % (k, float((err / np.maximum(bnd, 1e-300)).max()))
        # the bound is a rounding bound, not a tolerance: a few u of the value (the quotient by a small denominator aside)
        assert (bnd <= 64 * L.U * (np.abs(r) + np.abs(p) + 1e-30)).mean() > 0.95, k


def test_adam64_is_torch_adam_in_float64():
    """The same update by torch.optim.Adam on float64 tensors, at the step count torch is told to be at."""
    for betas, wd, step in [((0.9, 0.999), 5e-5, 0), ((0.5, 0.999), 0.0, 7), ((0.0, 0.5), 5e-5, 999)]:
        p, g, m, v = L.adam_state(257, seed=9, steps_done=step)
        lr = float(np.float32(1e-3))
        tp = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
        opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=float(np.float32(1e-8)), weight_decay=float(np.float32(wd)))
        opt.state[tp] = {"step": torch.tensor(float(step)), "exp_avg": torch.tensor(m, dtype=torch.float64),
                         "exp_avg_sq": torch.tensor(v, dtype=torch.float64)}
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        ref = L.adam64(p, g, m, v, step, np.float32(1e-3), betas[0], betas[1], 1e-8, wd)
        # the kernel's coefficients are fp32 roundings of torch's doubles: agreement to a few fp32 roundings of the update
        upd = np.abs(ref["p"][0] - p.astype(np.float64))
        assert (np.abs(ref["p"][0] - tp.detach().numpy()) <= 8 * L.U * (upd + 1e-12)).all()
        assert (np.abs(ref["m"][0] - opt.state[tp]["exp_avg"].numpy()) <= 4 * L.U * (np.abs(ref["m"][0]) + np.abs(g) + np.abs(m))).all()
        assert (np.abs(ref["v"][0] - opt.state[tp]["exp_avg_sq"].numpy()) <= 4 * L.U * (np.abs(ref["v"][0]) + 1e-30)).all()


def test_adam_coefficients_follow_the_kernel():
    assert L.pow_int(0.999, 1000) == pytest.approx(0.999 ** 1000, rel=1e-13)
    assert L.pow_int(0.0, 1) == 0.0 and L.pow_int(0.5, 0) == 1.0
    s, b = L.adam_coeffs(0.9, 0.999, 0, np.float32(1e-3))
    assert s.dtype == np.float32 and b.dtype == np.float32
    assert float(s) == float(np.float32(float(np.float32(1e-3)) / (1.0 - 0.9))) and float(b) == float(np.float32(np.sqrt(1.0 - 0.999)))
    s0, b0 = L.adam_coeffs(0.0, 0.5, 999, np.float32(1e-3))
    assert float(s0) == float(np.float32(1e-3)) and float(b0) == 1.0
    w1, b2, w2, eps, wd = L.adam_hyper(0.5, 0.999, 1e-8, 5e-5)
    assert not (w1 < np.float32(0.5)) and L.adam_hyper(0.9, 0.999, 1e-8, 0)[0] < np.float32(0.5)        # both lerp branches
