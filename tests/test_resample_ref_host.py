"""CPU checks of tests/resample_ref.py, the float64 reference under tests/test_resample_act.py: a reference that is wrong would pass
or fail the kernels for the wrong reason."""
import numpy as np
import pytest

from tests import resample_ref as R


@pytest.mark.parametrize("rows,cols,B,C,seed", [(27, 17, 5, 6, 1), (40, 9, 2, 3, 2)])
def test_spmm64_is_the_dense_product(rows, cols, B, C, seed):
    rowptr, col, val = R.make_csr(rows, cols, seed)
    x = np.random.default_rng(seed).standard_normal((cols, B, C)).astype(np.float32)
    y, absum = R.spmm64(rowptr, col, val, x)
    m = R.dense(rowptr, col, val, cols)
    ref = np.einsum("rk,kbc->rbc", m, x.astype(np.float64))
    assert np.abs(y - ref).max() <= 1e-13
    # absum bounds the sum and is the sum of the absolute terms (no repeated column merged away)
    assert (np.abs(y) <= absum + 1e-13).all()
    aref = np.zeros_like(absum)
    for r in range(rows):
        for e in range(rowptr[r], rowptr[r + 1]):
            aref[r] += np.abs(np.float64(val[e]) * x[col[e]].astype(np.float64))
    assert np.abs(absum - aref).max() <= 1e-13


def test_make_csr_holds_every_entry_count_and_a_row_select():
    rowptr, col, val = R.make_csr(27, 17, 3)
    cnt = R.row_counts(rowptr)
    assert rowptr.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float32
    assert rowptr[0] == 0 and rowptr[-1] == len(col) == len(val)
    assert set(cnt.tolist()) == set(R.COUNTS) == {0, 1, 2, 3, 4, 5, 7, 8, 9}
    assert col.min() >= 0 and col.max() < 17
    assert (val > 0).any() and (val < 0).any()
    assert any(len(set(col[rowptr[r]:rowptr[r + 1]].tolist())) < cnt[r] for r in range(27))              # a column repeats in a row
    sel = R.select_rows(rowptr, val)
    assert len(sel) >= 1 and all(cnt[r] == 1 and val[rowptr[r]] == 1.0 for r in sel)
    # the rows the GPU sweep zeroes are not the empty or the select rows (the zeroing must be what makes them 0)
    assert cnt[13] == 4 and cnt[26] == 9
    # the long matrices of the grid-stride cases keep the cycle
    assert set(R.row_counts(R.make_csr(4200, 17, 4)[0]).tolist()) == set(R.COUNTS)


def test_derivatives_from_the_output_match_the_activation_slopes():
    """dact64(act, act64(act, v)) is d act / d v (central difference in float64); the leaky slope is the fp32 constant."""
    v = np.linspace(-3.0, 3.0, 241) + 1e-3
    h = 1e-6
    for act in R.ACTS:
        num = (R.act64(act, v + h) - R.act64(act, v - h)) / (2 * h)
        d = R.dact64(act, R.act64(act, v))
        tol = 1e-7 if act != 3 else 2.0 ** -24                   # leaky: float32(0.02) against the double 0.02 the activation uses
        assert np.abs(num - d).max() <= tol, act
    assert R.LEAKY == float(np.float32(0.02)) and R.LEAKY != 0.02


def test_bf16_half_spacing_and_rounding():
    ref = np.array([0.0, 1.0, -1.0, 1.99, 2.0, 0.75, -3.0e-3, 130.0])
    hs = R.bf16_half_spacing(ref)
    assert hs[0] == 0.0
    assert hs[1] == hs[2] == hs[3] == 2.0 ** -8 and hs[4] == 2.0 ** -7 and hs[5] == 2.0 ** -9 and hs[7] == 2.0 ** -1
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4096) * np.exp(rng.uniform(-5, 5, 4096))
    a32 = a.astype(np.float32)
    back = R.bf16_np(R.to_bf16(a32))
    assert (np.abs(back - a32.astype(np.float64)) <= R.bf16_half_spacing(a32.astype(np.float64))).all()   # one round to nearest
    assert np.array_equal(R.bf16_np(R.to_bf16(back)), back)


def test_reference_bounds_are_zero_where_the_arithmetic_is_exact():
    rowptr, col, val = R.make_csr(27, 17, 5)
    rng = np.random.default_rng(5)
    x = R.normal((17, 2, 4), rng)
    s, absum = R.spmm64(rowptr, col, val, x)
    ref, bound = R.spmm_ref(rowptr, s, absum, zero_row=13)
    empty = np.flatnonzero(R.row_counts(rowptr) == 0)
    assert (ref[empty] == 0).all() and (bound[empty] == 0).all() and (ref[13] == 0).all() and (bound[13] == 0).all()
    for r in R.select_rows(rowptr, val):
        assert np.array_equal(ref[r], x[col[rowptr[r]]].astype(np.float64))
    dy, y = R.normal((5, 2, 4), rng), R.act_output(5, (5, 2, 4), rng)
    ref, bound = R.act_backward_ref(dy, y, 5, zero_row=4)
    assert (ref[4] == 0).all() and (bound[4] == 0).all() and (bound[:4] > 0).all()
    assert np.abs(y).max() < 1.0
