"""Which kernel the fp32 spiral-conv weight gradient launches, with which plan, and that the result is right - one row per regime of
choose_wgrad (csrc/spiral_conv.hip): the streaming kernel's batch slices, channel tiles, 3-channel and interleaved variants, the
vertex walks, layers of more than 128 output channels, the bf16x3 kernel and its fall-back, the staged kernel, and the pre-sum
job folded into the launch or launched on its own.

Every row pins the launches of one call as the dispatch record writes them: kernel name with its template arguments, and the
shape tag with the grid and the folded pre-sum rows.  A row that fails says the choice, the plan or the record name moved (the
benchmark's tables and the committed profiles read these names).  dW and dbias are compared with the oracle in float64
(oracle/ref_cpu.spiral_conv, identity activation) at test_gpu_parity's gradient tolerance; pre-summed rows bit for bit with
sh_spmm on the same inputs, their plane image with sh_spmm_p3's."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu
from semantichuman_amd import _lib, ops
from tests.launch_record import launches

pytestmark = pytest.mark.gpu
GRAD_TOL = 1e-4                      # as tests/test_gpu_parity.py: max-abs-err <= 1e-4 * max|reference|
SUM_ROWS = 20                        # rows of a pre-sum job


def row(name, shape, expect, mma="exact", dp_pad=0, presum=False, planes=False):
    return pytest.param(shape, mma, dp_pad, presum, planes, expect, id=name)


def stream(inst, R, B, K, N, grid, presum=0):
    return ("wgrad_stream_kernel<%s>" % inst, "R=%d B=%d K=%d N=%d grid=%d presum=%d" % (R, B, K, N, grid, presum))


def split3(cot, R, B, K, N, grid, presum=0):
    return ("wgrad_split3_kernel<%d>" % cot, "R=%d B=%d K=%d N=%d grid=%d presum=%d" % (R, B, K, N, grid, presum))


def staged(inst, R, B, K, N, grid):
    return ("wgrad_kernel<%s>" % inst, "R=%d B=%d K=%d N=%d grid=%d" % (R, B, K, N, grid))


REDUCE = ("slab_reduce_kernel", "")
ROWS = [
    # ---- streaming kernel <COT, NG, DEPTH, FULL, C3 | ilv>
    row("ng1-full", (4, 50, 5, 8, 16), [stream("1, 1, 3, true, false", 50, 4, 40, 16, 16), REDUCE]),
    row("ng1-ragged", (3, 50, 5, 8, 16), [stream("1, 1, 3, false, false", 50, 3, 40, 16, 16), REDUCE]),
    row("ng4-full-cot2-ilv", (16, 60, 9, 32, 32), [stream("2, 4, 3, true, ilv", 60, 16, 288, 32, 80), REDUCE]),
    row("ng4-ragged-cot4-ilv-plain-walk", (70, 33, 9, 32, 64), [stream("4, 4, 2, false, ilv", 33, 70, 288, 64, 207), REDUCE]),
    row("ng8", (32, 64, 9, 32, 16), [stream("1, 8, 3, true, false", 64, 32, 288, 16, 80), REDUCE]),
    row("cot8-ilv", (16, 40, 4, 16, 128), [stream("8, 4, 2, true, ilv", 40, 16, 64, 128, 16), REDUCE]),
    row("c3", (9, 77, 7, 3, 16), [stream("1, 4, 3, false, true", 77, 9, 21, 16, 24), REDUCE]),
    row("ilv-off-short-group", (16, 50, 5, 12, 20), [stream("2, 4, 3, true, false", 50, 16, 60, 20, 16), REDUCE]),
    row("ilv-off-dpre-stride", (16, 50, 5, 8, 32), [stream("2, 4, 3, true, false", 50, 16, 40, 32, 16), REDUCE], dp_pad=1),
    # ---- vertex walks: one range per XCD with 1 (above), 2, 4, 8 batch slices; the plain one with 3, and for <= 3 output channels
    row("xcd-2-slices", (32, 60, 9, 32, 32), [stream("2, 4, 3, true, ilv", 60, 32, 288, 32, 152), REDUCE]),
    row("xcd-4-slices", (64, 40, 5, 16, 32), [stream("2, 4, 3, true, ilv", 40, 64, 80, 32, 80), REDUCE]),
    row("xcd-8-slices", (128, 24, 3, 8, 32), [stream("2, 4, 3, true, ilv", 24, 128, 24, 32, 48), REDUCE]),
    row("plain-3-slices", (48, 40, 5, 16, 32), [stream("2, 4, 3, true, ilv", 40, 48, 80, 32, 60), REDUCE]),
    row("plain-thin-layer-ng8", (64, 100, 10, 16, 3), [stream("1, 8, 3, true, false", 100, 64, 160, 3, 150), REDUCE]),
    # ---- more than 128 output channels: one launch per group of 128, the last one short (132: a dpre row stride of 132 floats
    # is no multiple of 8, so the eight tiles of the first launch do not interleave either)
    row("cout-160", (16, 60, 6, 16, 160), [stream("8, 4, 2, true, ilv", 60, 16, 96, 160, 32),
                                           stream("2, 4, 3, true, ilv", 60, 16, 96, 160, 32), REDUCE]),
    row("cout-132", (3, 70, 3, 8, 132), [stream("8, 1, 2, false, false", 70, 3, 24, 132, 24),
                                         stream("1, 1, 3, false, false", 70, 3, 24, 132, 24), REDUCE]),
    # ---- bf16x3 kernel: 2 and 4 channel tiles of a whole 16-wide slice; everything else stays exact
    row("x3-cot2", (16, 60, 9, 32, 32), [split3(2, 60, 16, 288, 32, 80), REDUCE], mma="split3"),
    row("x3-cot4", (32, 40, 5, 16, 64), [split3(4, 40, 32, 80, 64, 40), REDUCE], mma="split3"),
    row("x3-ragged-batch-stays-exact", (20, 40, 5, 16, 32), [stream("2, 4, 3, false, ilv", 40, 20, 80, 32, 40), REDUCE], mma="split3"),
    row("x3-cout-160-per-launch", (16, 60, 6, 16, 160), [stream("8, 4, 2, true, ilv", 60, 16, 96, 160, 32),
                                                          split3(2, 60, 16, 96, 160, 32), REDUCE], mma="split3"),
    row("planes3-stays-exact", (16, 60, 9, 32, 32), [stream("2, 4, 3, true, ilv", 60, 16, 288, 32, 80), REDUCE], mma="planes3"),
    # ---- staged kernel <COT, CTW, false>: input channels neither a multiple of 4 nor 3
    row("staged-cot1", (2, 64, 4, 5, 7), [staged("1, 1, false", 64, 2, 20, 7, 4), REDUCE]),
    row("staged-cot1-ctw2", (2, 40, 5, 14, 16), [staged("1, 2, false", 40, 2, 70, 16, 3), REDUCE]),
    row("staged-cot2-ctw2", (2, 64, 5, 14, 32), [staged("2, 2, false", 64, 2, 70, 32, 4), REDUCE]),
    row("staged-cot4", (5, 40, 3, 5, 64), [staged("4, 1, false", 40, 5, 15, 64, 10), REDUCE]),
    row("staged-cot8", (3, 30, 3, 6, 128), [staged("8, 1, false", 30, 3, 18, 128, 4), REDUCE]),
    # ---- the pre-sum job: folded into the launch (presum=<rows> in the tag) or a launch of its own in front of it
    row("rider-folded-exact-cot4", (16, 60, 5, 16, 64), [stream("4, 4, 2, true, ilv", 60, 16, 80, 64, 32, SUM_ROWS), REDUCE], presum=True),
    row("rider-folded-x3-cot2", (16, 60, 5, 16, 32), [split3(2, 60, 16, 80, 32, 32, SUM_ROWS), REDUCE], mma="split3", presum=True),
    row("rider-own-launch-x3-cot4", (16, 60, 5, 16, 64), [("spmm_kernel<true>", "rows=20 B=16 C=64"), split3(4, 60, 16, 80, 64, 32), REDUCE],
        mma="split3", presum=True),
    row("rider-own-launch-c3", (16, 60, 7, 3, 16), [("spmm_kernel<true>", "rows=20 B=16 C=16"), stream("1, 4, 3, true, true", 60, 16, 21, 16, 16), REDUCE],
        presum=True),
    row("rider-own-launch-cout-18", (16, 50, 5, 8, 18), [("spmm_kernel<false>", "rows=20 B=16 C=18"), stream("2, 4, 3, true, false", 50, 16, 40, 18, 16), REDUCE],
        presum=True),
    row("rider-folded-with-plane-image", (16, 60, 5, 16, 32), [stream("2, 4, 3, true, ilv", 60, 16, 80, 32, 32, SUM_ROWS), REDUCE],
        presum=True, planes=True),
]


def _case(shape, dp_pad):
    """Inputs of a row and the oracle's float64 gradients.  dpre is vertex-major [R][B][Cout (+ dp_pad unused floats)]."""
    B, R, S, cin, cout = shape
    rs = np.random.RandomState(sum(p * q for p, q in zip(shape, (1, 3, 5, 7, 11))) % 1000)
    table = rs.randint(0, R, size=(R, S)).astype(np.int32)
    table[:, 0] = np.arange(R)
    table[rs.rand(R, S) < 0.15] = R - 1
    table[-1] = R - 1
    x = torch.from_numpy(rs.randn(B, R, cin).astype(np.float32))
    gy = torch.from_numpy(rs.randn(B, R, cout).astype(np.float32))
    gy[:, -1] = 0.0                                              # the oracle masks the dummy row's output
    Wo = torch.zeros(cout, S * cin, dtype=torch.float64, requires_grad=True)
    bo = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    yo = ref_cpu.spiral_conv(x.double(), torch.from_numpy(table.astype(np.int64))[None], Wo, bo, "identity")
    (yo * gy.double()).sum().backward()
    d = torch.device("cuda:0")
    dpre_buf = torch.zeros(R, B, cout + dp_pad, device=d)
    dpre_buf[:, :, :cout] = gy.permute(1, 0, 2).to(d)
    return dict(x=x.permute(1, 0, 2).contiguous().to(d), dpre_buf=dpre_buf, table=torch.from_numpy(table).to(d), dW=Wo.grad, db=bo.grad)


def _sum_job(R, rs):
    """A CSR matrix of SUM_ROWS rows over the R rows of dpre, 0..5 entries per row."""
    counts = rs.randint(0, 6, size=SUM_ROWS)
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    col = rs.randint(0, R, size=int(rowptr[-1])).astype(np.int32)
    val = rs.rand(int(rowptr[-1])).astype(np.float32)
    return tuple(torch.from_numpy(a).to("cuda:0") for a in (rowptr, col, val))


def close(got, ref, what):
    got, ref = got.double().cpu().numpy(), ref.numpy()
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print("%s: max-abs-err %.3e, bound %.3e" % (what, err, GRAD_TOL * scale))
    assert np.isfinite(got).all() and err <= GRAD_TOL * scale + 1e-30, what


@pytest.mark.parametrize("shape, mma, dp_pad, presum, planes, expect", ROWS)
def test_wgrad_form(shape, mma, dp_pad, presum, planes, expect):
    B, R, S, cin, cout = shape
    c = _case(shape, dp_pad)
    lib, d = _lib.load(), c["x"].device
    nbytes = lib.sh_spiral_conv_bwd_wgt_workspace(B, R, S, cin, cout)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=d)
    dW, db = torch.empty(cout, S * cin, device=d), torch.empty(cout, device=d)
    dsv, dsb = B * (cout + dp_pad), cout + dp_pad
    job = _sum_job(R, np.random.RandomState(R)) if presum else (None, None, None)
    out = torch.zeros(SUM_ROWS, B, cout, device=d) if presum else None
    img_bytes = SUM_ROWS * int(lib.sh_p3_bytes(1, B, cout)) if planes else 0
    img = torch.zeros(img_bytes, dtype=torch.uint8, device=d) if planes else None
    P = _lib.ptr

    def call():
        _lib.check(lib.sh_spiral_conv_bwd_wgt_presum(P(c["dpre_buf"]), dsv, dsb, P(c["x"]), B * cin, cin, P(c["table"]), P(dW), P(db), P(ws),
                                                     nbytes, P(job[0]), P(job[1]), P(job[2]), P(out), P(img), SUM_ROWS if presum else 0,
                                                     B, R, S, cin, cout, _lib.MMA_MODES[mma], _lib.stream_ptr()), "sh_spiral_conv_bwd_wgt_presum")

    _, rec = launches(call)
    print("launches:", rec)
    assert rec == expect
    close(dW, c["dW"], "dW")
    close(db, c["db"], "dbias")
    if presum:
        ref = torch.zeros_like(out)
        ops.spmm(job, c["dpre_buf"], "vm", ref, "vm", SUM_ROWS)
        assert torch.equal(out, ref)
    if planes:
        ref, ref_img = torch.zeros_like(out), torch.zeros_like(img)
        _lib.check(lib.sh_spmm_p3(P(job[0]), P(job[1]), P(job[2]), P(c["dpre_buf"]), dsv, dsb, P(ref), dsv, dsb, P(ref_img), None, 0, 0, 0, -1,
                                  B, SUM_ROWS, cout, _lib.stream_ptr()), "sh_spmm_p3")
        assert torch.equal(out, ref) and torch.equal(img, ref_img)
