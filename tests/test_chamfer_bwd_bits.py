"""The bytes of the Chamfer gradient, vertex form (sh_chamfer_bwd) and face form (sh_chamfer_surface_bwd), pinned against
tests/golden/chamfer_bwd_bits.json: the SHA-256 of g_x per configuration, recorded on an MI355X from the library of the commit
before the two kernels came to share a launcher and a source file (`SH_KERNEL_LIB=<that build> python -m tests.test_chamfer_bwd_bits <out.json>`).  The
order of the fp32 adds, the kept rule, the contraction of either form and every element stored are all in those bytes.

Inputs come from a seed; the match arrays are built by hand, not by a search, so that they hold what a search rarely gives:
48 kept scan points of one tile with the same active partner (vertex 5 / face 0), a face whose corners lie in two row tiles, face indices
-1 and >= nF, a face with a corner >= n, idx_sm entries -1 and n (the dummy row).  The entry points are called directly: M = 0
needs non-null pointers to nothing, which a tensor cannot give."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib
from semantichuman_amd._lib import ptr, stream_ptr

GOLD = os.path.join(os.path.dirname(__file__), "golden", "chamfer_bwd_bits.json")
DEV = "cuda:0"
B, N, ROWS, NF = 3, 300, 301, 500          # two row tiles, the second partial, and the dummy row
TAU2 = 0.667                               # d2 is uniform in [0, 1): about a third of the pairs is dropped
MS = (0, 1, 256, 257, 600)                 # no tile, one entry, exactly one tile, one + 1 (the prefetch's last-tile edge), two + a partial one
MASKS = ("none", "n", "Bn")
W_MS = (0.0, 0.5)
CASES = [(M, mask, w) for M in MS for mask in MASKS for w in W_MS]
case_id = lambda c: "M%d-mask_%s-w%g" % c


def inputs(M, mask, w_ms):
    """Host arrays of one configuration."""
    r = np.random.RandomState(1000 * M + 10 * MASKS.index(mask) + int(w_ms > 0))
    x = r.standard_normal((B, ROWS, 3)).astype(np.float32)
    x[:, N] = np.nan                                                       # the dummy row: a kernel that read it would show
    s = r.standard_normal((B, M, 3)).astype(np.float32)
    s_count = np.array([M, max(M - 7, 0), 0], np.int32)                    # all, fewer (where M allows), none
    faces = r.randint(0, N, (NF, 3)).astype(np.int32)
    faces[0] = (10, 270, 20)                                               # corners in both row tiles
    faces[1] = (3, N + 5, 7)                                               # a corner that is no vertex
    faces[2] = (N, 1, 2)                                                   # the dummy row as a corner
    idx_sm = r.randint(0, N, (B, M)).astype(np.int32)
    face = r.randint(0, NF, (B, M)).astype(np.int32)
    for k, (iv, fv) in enumerate(((-1, -1), (N, NF), (N + 9, NF + 3), (7, 1), (8, 2))):
        if M > 60 + k:
            idx_sm[:, 60 + k] = iv; face[:, 60 + k] = fv
    idx_sm[:, 2:50] = 5; face[:, 2:50] = 0                                 # 48 points of one tile with one partner (M allowing)
    idx_sm[:, 258:262] = 5; face[:, 258:262] = 0                           # and the same partner again in the next tile
    d2_sm = r.random_sample((B, M)).astype(np.float32)
    d2_sm[:, 2:50] = 0.1                                                   # all 48 are kept: 48 fp32 adds into one row, in order
    v = r.random_sample((B, M)).astype(np.float32)
    uv = np.stack([v, (r.random_sample((B, M)).astype(np.float32) * (np.float32(1) - v))], -1).astype(np.float32)
    idx_ms = r.randint(-1, M + 2, (B, ROWS)).astype(np.int32)              # -1, live, beyond the count and >= M
    d2_ms = r.random_sample((B, ROWS)).astype(np.float32)
    vm = {"none": None, "n": (r.random_sample(N) > 0.2), "Bn": (r.random_sample((B, N)) > 0.2)}[mask]
    vm = None if vm is None else vm.astype(np.uint8)
    if vm is not None:
        vm[..., [5, 10, 20, 270]] = 1                                      # the shared partner and face 0's corners stay active
    n_act = [N if vm is None else int((vm if vm.ndim == 1 else vm[b]).sum()) for b in range(B)]
    counts = np.array([[min(int(s_count[b]), M), n_act[b]] for b in range(B)], np.int32)   # what sh_chamfer_fwd leaves
    gL = r.standard_normal(B).astype(np.float32)
    return dict(x=x, s=s, s_count=s_count, faces=faces, idx_sm=idx_sm, face=face, d2_sm=d2_sm, uv=uv, idx_ms=idx_ms, d2_ms=d2_ms, vm=vm,
                counts=counts, gL=gL)


def dev(a):
    """The array on the device, one element longer than it is: an empty array still has an address."""
    t = torch.zeros(a.size + 1, dtype=torch.from_numpy(a[:0].ravel()).dtype, device=DEV)
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a).ravel()).to(DEV)
    return t


def gradients(M, mask, w_ms):
    """(g_x of the vertex form, g_x of the face form) as host bytes."""
    h = inputs(M, mask, w_ms)
    d = {k: (None if a is None else dev(a)) for k, a in h.items()}
    ms = (d["idx_ms"], d["d2_ms"]) if w_ms > 0 else (None, None)
    mask_sb = N if mask == "Bn" else 0
    lib = _lib.load()
    out = []
    for form in ("vertex", "face"):
        g = torch.full((B * ROWS * 3,), float("nan"), dtype=torch.float32, device=DEV)   # every element is to be written
        head = (ptr(d["x"]), 3 * ROWS, ROWS, N, ptr(d["s"]), 3 * M, M, ptr(d["s_count"]))
        tail = (ptr(ms[0]), ptr(ms[1]), ptr(d["vm"]), mask_sb, ptr(d["counts"]), TAU2, w_ms, ptr(d["gL"]), B, ptr(g), stream_ptr())
        if form == "vertex":
            _lib.check(lib.sh_chamfer_bwd(*head, ptr(d["idx_sm"]), ptr(d["d2_sm"]), *tail), "sh_chamfer_bwd")
        else:
            _lib.check(lib.sh_chamfer_surface_bwd(*head, ptr(d["faces"]), NF, ptr(d["face"]), ptr(d["d2_sm"]), ptr(d["uv"]), *tail),
                       "sh_chamfer_surface_bwd")
        out.append(g.cpu().numpy().tobytes())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gradient_bytes_are_the_recorded_ones(case):
    with open(GOLD) as f:
        gold = json.load(f)[case_id(case)]
    for form, g in zip(("vertex", "face"), gradients(*case)):
        a = np.frombuffer(g, np.float32).reshape(B, ROWS, 3)
        assert np.isfinite(a).all(), form                                  # every element written, the dummy row never read
        assert not a[:, N].any() and not a[2].any(), form                  # no gradient for the dummy row, nor without scan points
        assert hashlib.sha256(g).hexdigest() == gold[form], (form, case_id(case))


if __name__ == "__main__":                                                 # the recording (see the module's text)
    rec = {case_id(c): dict(zip(("vertex", "face"), (hashlib.sha256(g).hexdigest() for g in gradients(*c)))) for c in CASES}
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("recorded %d configurations with %s" % (len(rec), _lib.LIB_PATH))
