"""The depth field and the free-space term without a GPU: the host reference of tests/field_ref.py against itself (two-pass form
against brute force) and against truth (analytic tie cases, the float64 derivative), the ValueErrors of scan.DepthField,
scan.free_space and the fits, and the argument checks of the C entry points, which return before the device is touched."""
import ctypes
import math

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, editing, scan
from tests import field_ref as R


@pytest.mark.parametrize("seed", range(6))
def test_two_pass_form_equals_brute_force_on_random_masks(seed):
    """Sparse and dense random class images: integer distances tie all the time on a small grid."""
    rng = np.random.default_rng(seed)
    H, W = [(9, 14), (14, 9), (1, 17), (17, 1), (12, 12), (7, 23)][seed]
    for density in (0.03, 0.2, 0.7):
        cls = rng.choice(np.asarray([R.EMPTY, R.UNKNOWN, R.SURFACE], np.uint8), size=(H, W), p=[1 - density, density / 2, density / 2])
        assert np.array_equal(R.nearest_two_pass(cls), R.nearest_brute(cls))


def test_analytic_tie_cases():
    m = R.tie_masks()
    corners = R.nearest_brute(m["corners"])
    assert corners[2, 2] == 0 and corners[2, 3] == 4 and corners[3, 2] == 20 and corners[3, 3] == 24
    assert corners[2, 1] == 0 and corners[1, 2] == 0                       # (1, 2): 0 and 4 tie; (2, 1): 0 and 20 tie
    assert (R.nearest_brute(m["single"]) == 5 * 9 + 6).all()
    assert (R.nearest_brute(m["none"]) == -1).all()
    assert np.array_equal(R.nearest_brute(m["all"]), np.arange(24, dtype=np.int32).reshape(4, 6))
    assert R.nearest_brute(m["row_tie"])[6, 6] == 6 * 13 + 1               # not 11 * 13 + 6, equally far
    assert R.nearest_brute(m["column_tie"])[5].tolist() == [2 * 3 + 1] * 3
    for name, cls in m.items():
        assert np.array_equal(R.nearest_two_pass(cls), R.nearest_brute(cls)), name


def test_classification():
    depth = np.asarray([[0.0, np.nan, np.inf, -1.0, 9.0, 2.0, 0.2, 2.0]], np.float32)
    mask = np.asarray([[1, 1, 1, 1, 1, 1, 1, 0]])
    cls, z = R.classify(depth, mask=mask, z_range=(0.5, 5.0))
    U, E, S = R.UNKNOWN, R.EMPTY, R.SURFACE
    assert cls.tolist() == [[U, U, U, U, E, S, U, E]]                      # 0.2: nearer than z_near - it may hide the body
    assert z.tolist() == [[0, 0, 0, 0, 0, 2.0, 0, 0]]
    words = np.asarray([[0, 2000, 40000, 9000]], np.uint16)
    cls, z = R.classify(words, depth_scale=0.001, z_range=(0.5, 5.0))
    assert cls.tolist() == [[U, S, E, E]] and z[0, 1] == np.float32(2000) * np.float32(0.001)


def test_reference_is_defined_where_a_vertex_taken_as_it_is_and_an_identity_map_part():
    """R.edge_rows on a principal pixel of every class: Z = +inf keeps the case list (e = -inf: no term; an EMPTY pixel: an
    infinite offset from the ray, or no term without an allowed pixel), X = -inf and X = NaN are outside, and the kind-1 row's zero
    gradient words take the sign of gL.  No NaN anywhere in term, gradient or loss, and no warning."""
    import warnings
    want = {"surface": [R.NONE, R.OUTSIDE, R.OUTSIDE, R.FREE], "empty": [R.SILHOUETTE, R.OUTSIDE, R.OUTSIDE, R.SILHOUETTE],
            "none": [R.NONE, R.OUTSIDE, R.OUTSIDE, R.NONE]}
    for name, f in R.edge_fields().items():
        kinds = want[name]
        x = R.edge_rows(f)
        assert np.isposinf(x[0, 2]) and np.isneginf(x[1, 0]) and np.isnan(x[2, 0]) and x[3, 0] == 0 and np.signbit(x[3, 0])
        for gL in ((1.0, 1.0), (-2.0, -0.5)):
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                term, kind, g, counts = R.terms(x, len(x), f, None, 0.01)
                gx = R.gradient(kind, g, counts, gL, len(x) + 1)
                loss = R.losses(term, kind, counts)
            assert kind.tolist() == kinds and counts.tolist() == [4, kinds.count(R.FREE), kinds.count(R.SILHOUETTE), 2], name
            assert not np.isnan(term).any() and not np.isnan(gx).any() and not np.isnan(loss).any(), name
            assert (term[kind == R.NONE] == 0).all() and (gx[:4][np.isin(kind, (R.NONE, R.OUTSIDE))] == 0).all() and (gx[-1] == 0).all()
            if name == "surface":                                          # g = (0, 0, -2 e): the zeros carry the sign of gL[0] / n_act
                assert term[3] > 0 and (gx[3, :2] == 0).all() and np.signbit(gx[3, :2]).tolist() == [gL[0] < 0] * 2
                assert gx[3, 2] != 0 and np.signbit(gx[3, 2]) == (gL[0] > 0)
            if name == "empty":                                            # Z = +inf: rx, ry and the term are infinite, nothing is 0 * inf
                assert np.isposinf(term[0]) and np.isinf(gx[0]).all() and loss[1] == math.inf and loss[0] == 0.0


def constructed_vertices(f, rng, n):
    """n camera-frame vertices that project at least 0.25 pixel from every pixel boundary, half of them onto SURFACE pixels (in
    front of and behind the surface, |e| > 1e-3) and half onto EMPTY ones."""
    H, W = f.cls.shape
    fx, fy, cx, cy = (float(t) for t in f.intr)
    sv, su = np.nonzero(f.cls == R.SURFACE)
    ev, eu = np.nonzero(f.cls == R.EMPTY)
    pick_s, pick_e = rng.integers(0, sv.size, n // 2), rng.integers(0, ev.size, n - n // 2)
    u = np.concatenate([su[pick_s], eu[pick_e]]) + rng.uniform(-0.25, 0.25, n)
    v = np.concatenate([sv[pick_s], ev[pick_e]]) + rng.uniform(-0.25, 0.25, n)
    zs = f.z[sv[pick_s], su[pick_s]].astype(np.float64)
    e = rng.uniform(0.002, 0.3, n // 2) * rng.choice([-1.0, 1.0], n // 2)
    Z = np.concatenate([zs - e, rng.uniform(1.0, 3.0, n - n // 2)])
    return np.stack([(u - cx) / fx * Z, (v - cy) / fy * Z, Z], 1).astype(np.float32)


def test_float32_gradient_is_the_derivative_of_the_float64_restatement():
    """The tolerance: term and gradient are a handful of fp32 operations (each within 2^-24 relative) on |X|, |Y|, |Z| <= 3 and
    |a|, |b| <= 1; the worst absolute error is the cancellation in rx = X - a Z, 3 * 2^-24 * 3 ~ 5e-7, doubled by g = 2 rx and
    once more through a rx + b ry: 2.5e-6 bounds every component with room.  The float64 derivative is a central difference with
    h = 1e-6 of a function that is quadratic in the vertex while the pixel stays the same: its truncation error is zero and its
    rounding error ~ 1e-16 * term / h < 1e-9."""
    H, W = 24, 32
    intr = (40.0, 42.0, 15.25, 11.5)
    rng = np.random.default_rng(5)
    cls = np.zeros((H, W), np.uint8)
    cls[6:18, 10:22] = R.SURFACE
    cls[0:3, 0:5] = R.UNKNOWN
    f = R.field_of_classes(cls, intr, z=2.0 + 0.01 * rng.standard_normal((H, W)))
    n = 400
    x = constructed_vertices(f, rng, n)
    uf, vf, inside, u, v = R.project(x, f.intr, H, W)
    assert inside.all()                                                    # the construction, asserted: nothing has to be excluded
    assert (np.abs(uf - u) <= 0.25 + 1e-4).all() and (np.abs(vf - v) <= 0.25 + 1e-4).all()
    on_surface = f.cls[v, u] == R.SURFACE
    assert on_surface[:n // 2].all() and (f.cls[v, u][n // 2:] == R.EMPTY).all()
    assert (np.abs(f.z[v, u].astype(np.float64) - x[:, 2])[on_surface] > 1e-3).all()
    term, kind, g, counts = R.terms(x, n, f)
    assert set(kind.tolist()) == {R.NONE, R.FREE, R.SILHOUETTE} and counts.tolist()[0] == n
    h = 1e-6
    x64 = x.astype(np.float64)
    for k in range(3):
        step = np.zeros(3)
        step[k] = h
        hi, lo = R.terms64(x64 + step, n, f), R.terms64(x64 - step, n, f)
        d = ((hi[0] + hi[1]) - (lo[0] + lo[1])) / (2 * h)
        assert np.abs(g[:, k].astype(np.float64) - d).max() <= 2.5e-6
    t64 = R.terms64(x64, n, f)
    assert np.abs(term.astype(np.float64) - (t64[0] + t64[1])).max() <= 2.5e-6
    # the scaled gradient: the factor of the header, and zeros in the rows beyond n
    gx = R.gradient(kind, g, counts, (0.5, 2.0), n + 3)
    assert (gx[n:] == 0).all() and np.allclose(gx[:n][kind == R.FREE], 0.5 / n * g[kind == R.FREE], rtol=1e-6)


def test_render_sees_a_triangle():
    """A fronto-parallel triangle at z = 2 over a background at 9: the pixels inside it read 2, the rest 9."""
    tri = np.asarray([[-0.5, -0.5, 2.0], [0.5, -0.5, 2.0], [-0.5, 0.5, 2.0]])
    depth = R.render(tri, [[0, 1, 2]], (20.0, 20.0, 15.5, 11.5), 24, 32, 9.0, samples=40)
    assert depth[7, 11] == 2.0 and depth[15, 11] == 2.0 and depth[7, 19] == 2.0 and depth[15, 19] == 9.0 and depth[0, 0] == 9.0
    assert 40 <= (depth == 2.0).sum() <= 80                                # half of a 10 x 10 pixel square


FIELD = scan.DepthField(torch.zeros((2, 3, 4), dtype=torch.uint8), torch.zeros((2, 3, 4)), torch.zeros((2, 3, 4), dtype=torch.int32),
                        torch.ones((2, 4)))


def test_depth_field_fields_and_select():
    assert len(FIELD) == 2 and FIELD.shape == (3, 4)
    one = FIELD.select(slice(1, 2))
    assert len(one) == 1 and one.shape == (3, 4) and one.intrinsics.shape == (1, 4) and one.nearest.shape == (1, 3, 4)


@pytest.mark.parametrize("kwargs, match", [
    (dict(depth=np.zeros((2, 3, 4, 5), np.float32)), "depth must be"),
    (dict(depth=np.zeros((3, 4), np.float64)), "depth must be"),
    (dict(depth=np.zeros((0, 4), np.float32)), "depth must be"),
    (dict(intrinsics=(1.0, 1.0, 0.0)), "intrinsics must be"),
    (dict(intrinsics=(0.0, 1.0, 0.0, 0.0)), "fx and fy"),
    (dict(intrinsics=(1.0, math.inf, 0.0, 0.0)), "fx and fy"),
    (dict(mask=np.ones((4, 3), bool)), "mask must be"),
    (dict(mask=np.ones((3, 4), np.float32)), "mask must be"),
    (dict(z_range=(2.0, 1.0)), "z_range"),
    (dict(z_range=(1.0,)), "z_range"),
])
def test_depth_field_value_errors_before_any_device_use(kwargs, match):
    """The checks and messages of unproject_depth: one helper serves both."""
    args = dict(depth=np.ones((3, 4), np.float32), intrinsics=(10.0, 10.0, 2.0, 1.5))
    args.update(kwargs)
    depth, intrinsics = args.pop("depth"), args.pop("intrinsics")
    with pytest.raises(ValueError, match=match) as ours:
        scan.DepthField.from_depth(depth, intrinsics, "cuda:0", **args)
    with pytest.raises(ValueError, match=match) as theirs:
        scan.unproject_depth(depth, intrinsics, **args)
    assert str(ours.value).split(": ", 1)[1] == str(theirs.value).split(": ", 1)[1]


def test_fit_value_errors_before_any_device_use():
    """A field of another batch size, negative weights, a negative margin - checked before the model or the device is looked at."""
    z = torch.zeros((3, 4, 8))
    clouds = [np.zeros((5, 3), np.float32)] * 3
    scans = scan.ScanBatch._from_parts(torch.zeros((3, 5, 3)), torch.full((3,), 5, dtype=torch.int32), np.full(3, 5), None, None)
    three = scan.DepthField(torch.zeros((3, 3, 4), dtype=torch.uint8), torch.zeros((3, 3, 4)), torch.zeros((3, 3, 4), dtype=torch.int32),
                            torch.ones((3, 4)))
    del clouds
    for fit in (editing.fit_scan, editing.register_scan):
        with pytest.raises(ValueError, match="3 bodies, a field of 2 images"):
            fit(None, z, None, scans, free_space=FIELD)
        with pytest.raises(ValueError, match="free_space_weight must be >= 0"):
            fit(None, z, None, scans, free_space=three, free_space_weight=-1.0)
        with pytest.raises(ValueError, match="silhouette_weight must be >= 0"):
            fit(None, z, None, scans, free_space=three, silhouette_weight=-0.5)
        with pytest.raises(ValueError, match="margin must be >= 0"):
            fit(None, z, None, scans, free_space=three, free_space_margin=-1e-3)
        with pytest.raises(ValueError, match="must be a scan.DepthField"):
            fit(None, z, None, scans, free_space=(1, 2, 3))
    with pytest.raises(ValueError, match="free_space_pose must be"):
        editing.fit_scan(None, z, None, scans, free_space=three, free_space_pose=scan.Pose.identity(2, "cpu"))


def test_argument_validation_without_gpu():
    """The three entry points refuse bad arguments before they touch the device."""
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)                      # `p`: not null, never dereferenced on these paths
    inf = math.inf
    field = lambda depth=p, dtype=0, intr=p, B=1, H=4, W=4, cls=p, z=p, nearest=p, ws=p, nbytes=1 << 20: lib.sh_depth_field(
        depth, dtype, 1.0, intr, null, B, H, W, -inf, inf, cls, z, nearest, ws, nbytes, null)
    for rc in (field(depth=null), field(intr=null), field(cls=null), field(z=null), field(nearest=null)):
        assert rc == -1 and b"null pointer" in lib.sh_last_error()
    for rc in (field(B=-1), field(H=-1), field(W=-2)):
        assert rc == -1 and b"negative size" in lib.sh_last_error()
    assert field(dtype=2) == -1 and b"dtype" in lib.sh_last_error()
    for rc in (field(ws=null), field(nbytes=4 * 4 * 2 - 1)):
        assert rc == -1 and b"workspace" in lib.sh_last_error()
    for rc in (field(H=16385), field(W=16385, H=1)):
        assert rc == -2 and b"16384" in lib.sh_last_error()
    assert field(B=0) == 0 and field(H=0) == 0 and field(W=0) == 0         # nothing to do, nothing launched
    assert lib.sh_depth_field_workspace(2, 17, 33) == 2 * 17 * 33 * 2 and lib.sh_depth_field_workspace(0, 17, 33) == 0

    def fwd(x=p, x_sb=30, rows=10, n=9, cls=p, nearest=p, intr=p, H=4, W=4, mask=null, mask_sb=0, margin=0.0, B=2, term=p, counts=p):
        return lib.sh_free_space_fwd(x, x_sb, rows, n, cls, p, nearest, intr, H, W, mask, mask_sb, margin, B, term, p, p, counts, null)

    def bwd(x=p, x_sb=30, rows=10, n=9, H=4, W=4, mask=null, mask_sb=0, margin=0.0, counts=p, gL=p, B=2, g=p):
        return lib.sh_free_space_bwd(x, x_sb, rows, n, p, p, p, p, H, W, mask, mask_sb, margin, counts, gL, B, g, null)

    for rc in (fwd(x=null), fwd(cls=null), fwd(nearest=null), fwd(intr=null), fwd(term=null), fwd(counts=null), bwd(x=null), bwd(counts=null),
               bwd(gL=null), bwd(g=null)):
        assert rc == -1 and b"null pointer" in lib.sh_last_error()
    for rc in (fwd(B=-1), fwd(n=11), fwd(rows=-1, n=-1), fwd(H=-1), bwd(n=11), bwd(W=-1)):
        assert rc == -1 and b"bad size" in lib.sh_last_error()
    for rc in (fwd(margin=-1.0), fwd(margin=math.nan), bwd(margin=-0.5)):
        assert rc == -1 and b"margin" in lib.sh_last_error()
    for rc in (fwd(x_sb=26), bwd(x_sb=0)):
        assert rc == -1 and b"batch stride" in lib.sh_last_error()
    for rc in (fwd(mask=p, mask_sb=8), bwd(mask=p, mask_sb=1)):
        assert rc == -1 and b"mask stride" in lib.sh_last_error()
    for rc in (fwd(H=0), bwd(W=0)):
        assert rc == -1 and b"empty image" in lib.sh_last_error()
    for rc in (fwd(H=16385), bwd(W=20000)):
        assert rc == -2 and b"16384" in lib.sh_last_error()
    assert fwd(B=0) == 0 and bwd(B=0) == 0 and bwd(rows=0, n=0) == 0       # nothing to do, nothing launched
