"""Host-built transposed lists of the measurement gradients (measure.GirthRings / measure.Bones) and argument validation of
the three gradient entry points - no GPU needed."""
import ctypes
import os

import numpy as np
import pytest

from semantichuman_amd import _lib
from semantichuman_amd import constants as C
from semantichuman_amd import measure


def golden_rings():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "measure.npz"))
    n = int(g["n_planes"])
    return [g["factor_%d" % i] for i in range(n)], [g["epi_%d" % i] for i in range(n)]


def synthetic_rings():
    """n = 1, n = 2, a ring with a repeated point, a point whose two ends are the same vertex, a ring sharing vertices."""
    fac = [np.float32([0.5]), np.float32([0.25, 0.75]), np.float32([0.1, 0.1, 0.6, 0.3]), np.float32([0.5, 0.2, 0.9])]
    epi = [np.array([[4, 5]]), np.array([[0, 1], [2, 3]]), np.array([[6, 7], [6, 7], [8, 9], [7, 9]]), np.array([[3, 3], [1, 9], [9, 2]])]
    return fac, epi


RING_SETS = {"golden": golden_rings, "synthetic": synthetic_rings}


@pytest.mark.parametrize("which", sorted(RING_SETS))
def test_girth_lists_invert_the_forward_tables(which):
    fac, epi = RING_SETS[which]()
    r = measure.GirthRings(fac, epi, "cpu")
    ptr, a, b, f = (t.numpy() for t in r.tables())
    pt_ring, vt_ptr, vt_pt, vt_w, rows = r.transposed()
    pt_ring, vt_ptr, vt_pt, vt_w = (t.numpy() for t in (pt_ring, vt_ptr, vt_pt, vt_w))
    assert rows == r.max_vertex + 1 and vt_ptr.shape == (rows + 1,) and vt_ptr[0] == 0 and vt_ptr[-1] == 2 * r.n_points
    assert vt_ptr.dtype == np.int32 and vt_pt.dtype == np.int32 and vt_w.dtype == np.float32
    # ring of every point
    for p in range(r.n_rings):
        assert np.all(pt_ring[ptr[p]:ptr[p + 1]] == p)
    # forward entries: (vertex, point, weight) with weight 1 - f for a, f for b (the forward's fp32 arithmetic)
    fwd = sorted([(int(a[k]), k, 0, float(np.float32(1) - f[k])) for k in range(r.n_points)]
                 + [(int(b[k]), k, 1, float(f[k])) for k in range(r.n_points)])
    back = []
    for v in range(rows):
        ks = vt_pt[vt_ptr[v]:vt_ptr[v + 1]]
        assert np.all(np.diff(ks) >= 0)                                 # a row's entries in point order (the summation order)
        back += [(v, int(k), float(w)) for k, w in zip(ks, vt_w[vt_ptr[v]:vt_ptr[v + 1]])]
    assert [(v, k, w) for v, k, _, w in fwd] == back                    # exact inverse, same bits of every weight


@pytest.mark.parametrize("skl", ["SKL_LIST[1:]", "NEWSKL_LIST", "mixed"])
def test_bone_lists_invert_the_bone_table(skl):
    bl = {"SKL_LIST[1:]": C.SKL_LIST[1:], "NEWSKL_LIST": C.NEWSKL_LIST, "mixed": [[0, 1], [2, 3, 3], [1, 0], [4, 2, 5]]}[skl]
    bones = measure.Bones(bl, "cpu")
    t = bones.table.numpy()
    assert t.tolist() == measure.bone_table(bl, "cpu").tolist()
    jt_ptr, jt_bone, jt_w, rows = bones.transposed()
    jt_ptr, jt_bone, jt_w = jt_ptr.numpy(), jt_bone.numpy(), jt_w.numpy()
    assert rows == int(np.max([max(s) for s in bl])) + 1 and jt_ptr[-1] == sum(len(s) for s in bl)
    fwd = []
    for p, s in enumerate(bl):
        fwd.append((s[0], p, 0, 1.0))
        if len(s) == 2:
            fwd.append((s[1], p, 1, -1.0))
        else:
            fwd += [(s[1], p, 1, -0.5), (s[2], p, 2, -0.5)]
    fwd.sort()
    back = []
    for j in range(rows):
        ps = jt_bone[jt_ptr[j]:jt_ptr[j + 1]]
        assert np.all(np.diff(ps) >= 0)
        back += [(j, int(p), float(w)) for p, w in zip(ps, jt_w[jt_ptr[j]:jt_ptr[j + 1]])]
    assert [(j, p, w) for j, p, _, w in fwd] == back
    # the weights of each bone sum to 0 (a translation of all joints moves no length)
    sums = np.zeros(len(bl))
    np.add.at(sums, jt_bone, jt_w)
    assert np.all(sums == 0)


def _lib_or_build():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_gradient_entry_points_validate_without_gpu():
    lib = _lib_or_build()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                               # a host address: never dereferenced by a rejected call
    # null pointers
    assert lib.sh_measure_girth_bwd(null, 3, p, p, p, p, p, p, p, p, 1, p, 1, 1, 1, p, null) == -1
    assert b"null pointer" in lib.sh_last_error()
    assert lib.sh_measure_girth_bwd(p, 3, p, p, p, p, p, p, p, p, 1, p, 1, 1, 1, null, null) == -1
    assert lib.sh_bone_length_bwd(p, p, null, p, p, 1, p, 1, 2, 1, p, null) == -1
    assert b"null pointer" in lib.sh_last_error()
    assert lib.sh_joint_regress_bwd(p, null, 1, 2, 1, 3, p, null) == -1
    assert b"null pointer" in lib.sh_last_error()
    # bad sizes
    assert lib.sh_measure_girth_bwd(p, 30, p, p, p, p, p, p, p, p, 1, p, 0, 1, 10, p, null) == -1     # B = 0
    assert b"bad size" in lib.sh_last_error()
    assert lib.sh_measure_girth_bwd(p, 30, p, p, p, p, p, p, p, p, 11, p, 1, 1, 10, p, null) == -1    # table covers more rows
    assert lib.sh_measure_girth_bwd(p, 29, p, p, p, p, p, p, p, p, 5, p, 2, 1, 10, p, null) == -1     # batch stride < rows * 3
    assert lib.sh_bone_length_bwd(p, p, p, p, p, 3, p, 1, 2, 1, p, null) == -1                       # joints in table > K
    assert b"bad size" in lib.sh_last_error()
    assert lib.sh_bone_length_bwd(p, p, p, p, p, 1, p, 1, 2, 0, p, null) == -1                       # P = 0
    assert lib.sh_joint_regress_bwd(p, p, 1, 4, 1, 3, p, null) == -1                                 # rows < N
    assert b"bad size" in lib.sh_last_error()
    assert lib.sh_joint_regress_bwd(p, p, 1, 4, 0, 4, p, null) == -1                                 # K = 0


def test_differentiable_measurements_have_no_cpu_path():
    import torch
    fac, epi = golden_rings()
    r = measure.GirthRings(fac, epi, "cpu")
    v = torch.zeros((2, 579, 3), requires_grad=True)
    with pytest.raises(RuntimeError):
        measure.girths(v, r)
    with pytest.raises(RuntimeError):
        measure.bone_lengths(torch.zeros((2, 35, 3)), measure.Bones(C.SKL_LIST[1:], "cpu"))
    with pytest.raises(RuntimeError):
        measure.joints(torch.zeros((2, 579, 3)), torch.zeros((35, 578)))
    with pytest.raises(IndexError):
        measure.girths(torch.zeros((2, 50, 3)), r)
