"""isocontour(), tessellate() and render_figure() on `fem2d` surfaces in R^3 on the device against the NumPy twin
(tests/manifold_twin.py).

The combinatorial part of a result (`S` / `T`, `level`, `element`) must agree exactly once no lattice value is within
1024 eps max|z| of a level; that input condition is asserted on the twin alone (and without a GPU in
tests/test_manifold_post.py, where the cases live).  Level-curve vertices are compared against the per-vertex bound of
tests/test_gpu_contour.py,

    DEVICE_FACTOR p eps max|z| / |v_b - v_a| * |x_b - x_a|  +  8 eps max|x|,

and lattice triangles, whose vertices are plain sums of p products, against DEVICE_FACTOR p eps max|x| (positions) and
DEVICE_FACTOR p eps max|field| (values); DEVICE_FACTOR = 16 is imported from tests/test_gpu_interpolate_gradient.py.
"""
import ctypes as C

import numpy as np
import pytest

import mgb_amd as m
from helpers import record_observation
from manifold_twin import isocontour_twin_e, tessellate_twin
from mgb_amd.surface import TriangleCaster, composite_layers, default_surface_table, render_figure, render_surfaces
from mgb_amd.raycast import camera_rays
from test_contour import EPS, LEVELS1, LEVELS5, input_margin_ok, smooth
from test_gpu_interpolate_gradient import DEVICE_FACTOR
from test_manifold_post import FLAT_CASES, REFINES, SURFACE_CASES, flat_pair, sphere

pytestmark = pytest.mark.gpu


def _eq(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _same(c0, c1):
    return _eq(c0.points, c1.points) and _eq(c0.level, c1.level) and _eq(c0.element, c1.element) and _eq(c0.carried, c1.carried)


def _same_tess(t0, t1):
    return _eq(t0.points, t1.points) and _eq(t0.element, t1.element) and _eq(t0.values, t1.values)


@pytest.fixture(params=sorted(SURFACE_CASES), scope="module")
def case(request):
    geom = SURFACE_CASES[request.param]()
    z, carry = smooth(geom.xflat)
    return request.param, geom, z, carry


# ---------------------------------------------------------------------------------------------------------------------
# 1. isocontour against the twin
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_carry", [False, True], ids=["plain", "carry"])
@pytest.mark.parametrize("nlev", [1, 5])
@pytest.mark.parametrize("refine", REFINES, ids=lambda r: f"r{r}")
def test_isocontour_matches_the_twin(case, refine, nlev, with_carry):
    name, geom, z, carry = case
    levels = LEVELS1 if nlev == 1 else LEVELS5
    cr = carry if with_carry else None
    t = isocontour_twin_e(geom, z, levels, refine=refine, carry=cr)
    assert input_margin_ok(t, z), (name, refine, t.margin)
    c = m.isocontour(geom, z, levels, refine=refine, carry=cr)
    p = geom.x.shape[0]
    assert c.points.shape == (c.level.size, 2, 3) and c.points.dtype == np.float64
    assert c.level.dtype == np.int32 and c.element.dtype == np.int32
    assert c.level.size == t.level.size and c.level.size > 0, (name, c.level.size, t.level.size)
    assert np.array_equal(c.level, t.level) and np.array_equal(c.element, t.element)
    amp = DEVICE_FACTOR * p * EPS * np.abs(z).max() / t.dv
    bound = amp * t.dx + 8 * EPS * np.abs(geom.xflat).max()
    ratio = float((np.abs(c.points - t.points).max(axis=2) / bound).max())
    line = f"surface isocontour vs twin {name} refine={refine} nlev={nlev}: S = {c.level.size}, points error / bound {ratio:.3e}"
    if with_carry:
        assert c.carried.shape == (c.level.size, 2, 2)
        cbound = amp[..., None] * t.dc + 8 * EPS * np.abs(carry).max()
        cratio = float((np.abs(c.carried - t.carried) / cbound).max())
        line += f", carried error / bound {cratio:.3e}"
    else:
        assert c.carried is None
        cratio = 0.0
    print(line)
    record_observation(line)
    assert ratio <= 1.0 and cratio <= 1.0, line
    assert np.allclose(c.measure(), t.measure(), rtol=1e-9, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. tessellate against the twin
# ---------------------------------------------------------------------------------------------------------------------

def _check_tessellation(name, geom, fields, refine, ntri_per):
    p, N, e = geom.x.shape
    t = tessellate_twin(geom, fields, refine)
    c = m.tessellate(geom, fields, refine=refine)
    T = N * ntri_per
    assert c.points.shape == (T, 3, e) and c.points.dtype == np.float64
    assert c.element.shape == (T,) and c.element.dtype == np.int32
    assert t.points.shape == c.points.shape and np.array_equal(c.element, t.element)
    ratio = float(np.abs(c.points - t.points).max() / (DEVICE_FACTOR * p * EPS * np.abs(geom.xflat).max()))
    line = f"tessellate vs twin {name} refine={refine}: T = {T}, points error / bound {ratio:.3e}"
    vratio = 0.0
    if fields is None:
        assert c.values is None
    else:
        F = np.asarray(fields).reshape(p * N, -1)
        assert c.values.shape == (T, 3, F.shape[1])
        vratio = float((np.abs(c.values - t.values).max(axis=(0, 1)) / (DEVICE_FACTOR * p * EPS * np.abs(F).max(axis=0))).max())
        line += f", values error / bound {vratio:.3e}"
    print(line)
    record_observation(line)
    assert ratio <= 1.0 and vratio <= 1.0, line
    assert np.isclose(c.measure(), t.measure(), rtol=1e-9, atol=0)
    return c


@pytest.mark.parametrize("refine", REFINES, ids=lambda r: f"r{r}")
def test_tessellate_matches_the_twin_on_surfaces(case, refine):
    name, geom, z, carry = case
    r = geom.discretization.k if refine is None else refine
    F = np.concatenate([z[:, None], carry, geom.xflat[:, :2]], axis=1)          # five fields
    _check_tessellation(name, geom, F, refine, 2 * r * r)
    _check_tessellation(name, geom, z, refine, 2 * r * r)
    _check_tessellation(name, geom, None, refine, 2 * r * r)


@pytest.mark.parametrize("name", sorted(FLAT_CASES))
def test_tessellate_matches_the_twin_on_flat_meshes(name):
    make, other = FLAT_CASES[name]
    geom = make()
    z, carry = smooth(geom.xflat)
    default = {"fem2d_k2": 2, "fem2d_P1": 1, "fem2d_P2": 2}[name]
    for refine, r in ((None, default), (other, other)):
        ntri = 2 * r * r if name.startswith("fem2d_k") else r * r
        c = _check_tessellation(name, geom, np.concatenate([z[:, None], carry], axis=1), refine, ntri)
        assert abs(c.measure() - 4.0) <= 1e-12                                   # the square [-1, 1]^2
        _check_tessellation(name, geom, None, refine, ntri)


# ---------------------------------------------------------------------------------------------------------------------
# 3. embedding independence, bitwise
# ---------------------------------------------------------------------------------------------------------------------

def _old_entry(geom, z, levels, refine, carry):
    """`mgbhip_contour_create`, the entry without an ambient dimension, called through ctypes."""
    from mgb_amd.device import HipContext, _check, _ptr
    from mgb_amd.interpolate import _c_f64, _plan
    family, _, d, k, p, N, xnodes, table = _plan(geom)
    F = _c_f64(np.concatenate([z[:, None], carry], axis=1))
    lev, xnodes, table = _c_f64(np.asarray(levels, dtype=np.float64)), _c_f64(xnodes), _c_f64(table)
    ctx = HipContext(0)
    h, n = C.c_void_p(), C.c_int64(0)
    try:
        _check(ctx.lib, ctx.lib.mgbhip_contour_create(ctx.handle, family, d, k, p, N, _ptr(xnodes), _ptr(table), F.shape[1],
                                                      _ptr(F), lev.size, _ptr(lev), refine, C.byref(h), C.byref(n)))
        try:
            S = int(n.value)
            pts, car = np.empty((S, d, d)), np.empty((S, d, F.shape[1] - 1))
            lvl, elm = np.empty(S, np.int32), np.empty(S, np.int32)
            ip = C.POINTER(C.c_int32)
            _check(ctx.lib, ctx.lib.mgbhip_contour_fetch(h, _ptr(pts), lvl.ctypes.data_as(ip), elm.ctypes.data_as(ip), _ptr(car)))
        finally:
            ctx.lib.mgbhip_contour_destroy(h)
    finally:
        ctx.close()
    return pts, lvl, elm, car


@pytest.mark.parametrize("k", [1, 2])
def test_embedding_independence_is_bitwise(k):
    g2, g3 = flat_pair(k)
    z, carry = smooth(g2.xflat)
    for refine in (k, 3):
        a = m.isocontour(g2, z, LEVELS5, refine=refine, carry=carry)
        b = m.isocontour(g3, z, LEVELS5, refine=refine, carry=carry)
        assert a.level.size > 0 and a.points.shape[1:] == (2, 2) and b.points.shape[1:] == (2, 3)
        assert _eq(a.level, b.level) and _eq(a.element, b.element) and _eq(a.carried, b.carried)
        assert np.array_equal(b.points[..., :2], a.points) and np.all(b.points[..., 2] == 0.0)
        ta = m.tessellate(g2, np.concatenate([z[:, None], carry], axis=1), refine=refine)
        tb = m.tessellate(g3, np.concatenate([z[:, None], carry], axis=1), refine=refine)
        assert np.array_equal(tb.points[..., :2], ta.points) and np.all(tb.points[..., 2] == 0.0)
        assert _eq(ta.element, tb.element) and _eq(ta.values, tb.values)
        pts, lvl, elm, car = _old_entry(g2, z, LEVELS5, refine, carry)
        assert _eq(pts, a.points) and _eq(lvl, a.level) and _eq(elm, a.element) and _eq(car, a.carried)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the two kernels form the same lattice
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("refine", REFINES, ids=lambda r: f"r{r}")
def test_contour_vertices_lie_on_tessellation_edges_bitwise(case, refine):
    name, geom, z, carry = case
    tw = isocontour_twin_e(geom, z, LEVELS5, refine=refine)
    assert input_margin_ok(tw, z)
    c = m.isocontour(geom, z, LEVELS5, refine=refine, carry=carry)
    t = m.tessellate(geom, np.concatenate([z[:, None], carry], axis=1), refine=refine)
    assert c.level.size == tw.level.size
    i = tw.tri[:, None]
    assert np.array_equal(t.element[tw.tri], c.element)
    va, vb = t.values[i, tw.qa, 0], t.values[i, tw.qb, 0]
    s = (LEVELS5[c.level][:, None] - va) / (vb - va)
    xa, xb = t.points[i, tw.qa], t.points[i, tw.qb]
    assert np.array_equal(xa + s[..., None] * (xb - xa), c.points), name
    ca, cb = t.values[i, tw.qa, 1:], t.values[i, tw.qb, 1:]
    assert np.array_equal(ca + s[..., None] * (cb - ca), c.carried), name


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism
# ---------------------------------------------------------------------------------------------------------------------

def test_two_calls_are_bitwise_equal_and_ordered(case):
    name, geom, z, carry = case
    for refine in (None, 9):
        a = m.isocontour(geom, z, LEVELS5, refine=refine, carry=carry)
        b = m.isocontour(geom, z, LEVELS5, refine=refine, carry=carry)
        assert _same(a, b), name
        assert a.level.size > 0 and np.all(np.diff(a.element) >= 0)
        F = np.concatenate([z[:, None], carry], axis=1)
        ta, tb = m.tessellate(geom, F, refine=refine), m.tessellate(geom, F, refine=refine)
        assert _same_tess(ta, tb) and np.all(np.diff(ta.element) >= 0)
        for j in range(2):
            one = m.isocontour(geom, z, LEVELS5, refine=refine, carry=carry[:, j])
            assert _eq(one.carried[..., 0], a.carried[..., j]) and _eq(one.points, a.points), (name, j)
            tone = m.tessellate(geom, carry[:, j], refine=refine)
            assert _eq(tone.values[..., 0], ta.values[..., 1 + j]) and _eq(tone.points, ta.points), (name, j)


# ---------------------------------------------------------------------------------------------------------------------
# 6. rendering
# ---------------------------------------------------------------------------------------------------------------------

def test_render_figure_of_a_sphere():
    geom = sphere(2, 1)
    u, _ = smooth(geom.xflat)
    eye, target, size = (0.0, -4.0, 0.0), (0.0, 0.0, 0.0), (64, 48)
    W, H = size
    img = render_figure(geom, u, eye, target, size=size)
    assert img.shape == (H, W, 4) and img.dtype == np.float64
    tess = m.tessellate(geom, u)
    o, d = camera_rays(eye, target, (0, 0, 1), size, 30.0)
    clim = (float(u.min()), float(u.max()))
    with TriangleCaster(tess.points) as tc:
        hits = tc.trace(o, d, max_hits=1)
        layers = tc.shade(hits, d, tess.values[..., 0], default_surface_table(), clim, 0.3)
    by_hand = composite_layers(layers).reshape(H, W, 4)
    assert np.array_equal(img, by_hand)
    img2, depth = render_surfaces(tess, eye, target, size=size)
    assert np.array_equal(img, img2)
    assert np.array_equal(render_surfaces([tess], eye, target, size=size, values=tess.values[..., 0])[0], img)
    assert np.array_equal(render_figure(geom, u, eye, target, size=size, refine=1, volume=False), img)
    # the silhouette: the sphere covers the centre and not the corners
    for r, c in ((H // 2 - 1, W // 2 - 1), (H // 2, W // 2)):
        assert img[r, c, 3] == 1.0
    for r, c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert img[r, c, 3] == 0.0 and np.isinf(depth[r, c])
    # the flat facets lie inside the unit sphere by at most the sag of a facet with vertices on it: a triangle's
    # circumradius is at most (longest edge) / sqrt(3)
    P = tess.points
    ell = max(float(np.sqrt(((P[:, a] - P[:, b]) ** 2).sum(axis=1)).max()) for a, b in ((0, 1), (0, 2), (1, 2)))
    sag = 1.0 - np.sqrt(1.0 - ell * ell / 3.0)
    centre = float(depth[H // 2, W // 2])
    print(f"sphere m=2: longest edge {ell:.4f}, sag {sag:.4f}, centre depth {centre:.6f}")
    assert 3.0 <= centre <= 3.0 + sag
