"""TriangleCaster / RayCaster.render(layers=...) / render_figure on the device against the NumPy twin
(tests/surface_twin.py), which tests every ray against every triangle without a grid.

Both sides run the same IEEE operations without contraction, so `t`, `u` and `v` are compared bit for bit and the
triangle indices exactly, once no pair sits within 1e-9 of a decision (asserted on the twin alone in
tests/test_surface.py, where the cases live).  `shade` differs from the twin only in how the two sides round the
square root and the divisions of the normal: the bound is 16 eps max(1, max|table colour|) per channel.  The layered
render differs from the twin's merge only in `exp`, as the plain render does: `render_bound` with every layer counted
as one more step.
"""
import numpy as np
import pytest

import mgb_amd as m
from helpers import record_observation
from mgb_amd.raycast import RayCaster, camera_rays
from mgb_amd.surface import TriangleCaster, render_figure, render_surfaces
from raycast_twin import clip_box_twin, rays_twin
from surface_twin import composite_twin, normalize_twin, sample_margin, shade_twin, trace_twin
from test_raycast import CLIM, EPS, TABLE5, smooth
from test_surface import (GPU_CASES, HITS, MARGIN, NRAYS, UNIT, case_soup, rays65, soup_dup, soup_span, sphere_geom,
                          vertex_values)

pytestmark = pytest.mark.gpu

AMBIENT = 0.3


@pytest.fixture(params=sorted(GPU_CASES), scope="module")
def case(request):
    """One caster per case, shared by its tests, with the twin's hits for K = 8 (computed once, never modified)."""
    name = request.param
    pts, o, d, t_min, t_max, tie = case_soup(name)
    twin = trace_twin(pts, o, d, t_min, t_max, 8)[:4]
    for a in twin:
        a.setflags(write=False)
    with TriangleCaster(pts) as tc:
        yield name, pts, o, d, t_min, t_max, twin, tc


@pytest.mark.parametrize("K", HITS)
@pytest.mark.parametrize("R", NRAYS)
def test_trace_is_bitwise_the_twins(case, R, K):
    name, pts, o, d, t_min, t_max, twin, tc = case
    h = tc.trace(o[:R], d[:R], t_min, t_max, max_hits=K)
    t, tri, u, v = (a[:R, :K] for a in twin)               # the K nearest are the first K of the 8 nearest
    assert h.triangle.dtype == np.int32 and h.triangle.shape == (R, K) and h.t.dtype == np.float64
    assert np.array_equal(h.triangle, tri), (name, R, K)
    assert np.array_equal(h.t, t, equal_nan=True), (name, R, K)
    assert np.array_equal(h.u, u, equal_nan=True) and np.array_equal(h.v, v, equal_nan=True), (name, R, K)
    assert np.array_equal(np.isinf(h.t), tri < 0) and np.array_equal(np.isnan(h.u), tri < 0)
    again = tc.trace(o[:R], d[:R], t_min, t_max, max_hits=K)
    for a, b in ((h.t, again.t), (h.triangle, again.triangle), (h.u, again.u), (h.v, again.v)):
        assert np.array_equal(a, b, equal_nan=True), "two trace calls are bitwise equal"


def assert_hits_are_the_twins(h, twin, K, what):
    t, tri, u, v = (a[:, :K] for a in twin)                # the K nearest are the first K of the 8 nearest
    assert h.triangle.shape == (65, K) and np.array_equal(h.triangle, tri), what
    assert np.array_equal(h.t, t, equal_nan=True), what
    assert np.array_equal(h.u, u, equal_nan=True) and np.array_equal(h.v, v, equal_nan=True), what


@pytest.fixture(params=["dup", "random257"], scope="module")
def dispatch_case(request):
    name = request.param
    pts, o, d, t_min, t_max, tie = case_soup(name)
    twin = trace_twin(pts, o, d, t_min, t_max, 8)[:4]
    with TriangleCaster(pts) as tc:
        yield name, o, d, t_min, t_max, twin, tc


@pytest.mark.parametrize("K", range(1, 9))
def test_every_hit_count_is_bitwise_the_twins(dispatch_case, K):
    """Every case of the one dispatch over the hit count, at one full wave plus one lane."""
    name, o, d, t_min, t_max, twin, tc = dispatch_case
    assert_hits_are_the_twins(tc.trace(o, d, t_min, t_max, max_hits=K), twin, K, (name, K))


@pytest.fixture(scope="module")
def span_case():
    pts = soup_span()
    o, d = rays65(*UNIT)
    twin = trace_twin(pts, o, d, 0.02, 2.35, 8)[:4]
    with TriangleCaster(pts) as tc:
        yield o, d, twin, tc


@pytest.mark.parametrize("K", [1, 8])
def test_a_triangle_met_in_several_cells_is_kept_once(span_case, K):
    """A kept triangle is skipped before it is tested when a later cell lists it again: the hits are the twin's, which has
    no grid, bit for bit, and the large triangle (index 0) is among them (test_surface.py shows that on the twin)."""
    o, d, twin, tc = span_case
    h = tc.trace(o, d, 0.02, 2.35, max_hits=K)
    assert_hits_are_the_twins(h, twin, K, K)
    assert (h.triangle == 0).any(), "the large triangle is kept by some ray"
    for r in range(65):
        kept = h.triangle[r][h.triangle[r] >= 0]
        assert len(set(kept.tolist())) == kept.size, "no triangle is kept twice"


def test_ties_go_to_the_lower_index():
    """The deliberate ties, outside the margin condition: a duplicated triangle, and a ray through an edge that two
    triangles share bit for bit.  Both are hit, the lower index first, with the twin's bits."""
    a, b = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 0.0])
    edge = np.array([[a, [1.0, 0.0, 0.0], b], [a, b, [0.0, 1.0, 0.0]]])
    o, d = np.array([[0.5, 0.5, 2.0], [0.25, 0.25, -1.0]]), np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 3.0]])
    for pts, oo, dd in ((edge, o, d), (soup_dup(),) + case_soup("dup")[1:3]):
        t, tri, u, v, _ = trace_twin(pts, oo, dd, 0.0, np.inf, 2)
        with TriangleCaster(pts) as tc:
            h = tc.trace(oo, dd, max_hits=2)
        assert np.array_equal(h.triangle, tri) and np.array_equal(h.t, t, equal_nan=True)
        assert np.array_equal(h.u, u, equal_nan=True) and np.array_equal(h.v, v, equal_nan=True)
        tie = (h.triangle[:, 1] >= 0) & (h.t[:, 0] == h.t[:, 1])
        assert tie.any() and np.array_equal(h.triangle[tie], np.tile([0, 1], (tie.sum(), 1)))


def test_shade_matches_the_twin(case):
    name, pts, o, d, t_min, t_max, twin, tc = case
    t, tri, u, v = (a[:, :4] for a in twin)
    h = tc.trace(o, d, t_min, t_max, max_hits=4)
    vals = vertex_values(pts)
    table = TABLE5.copy()
    table[:, 3] = [0.0, 0.7, 1.3, 0.4, 1.0]                # alphas on both sides of the clamp
    got = tc.shade(h, d, vals, table, CLIM, AMBIENT)
    want = shade_twin(pts, normalize_twin(d), tri, u, v, vals, table, *CLIM, AMBIENT)
    bound = 16 * EPS * max(1.0, float(np.abs(table[:, :3]).max()))
    ratio = float(np.abs(got - want).max() / bound)
    record_observation(f"surface shade {name}: max difference / bound {ratio:.3e}")
    print(f"{name}: shade max difference / bound {ratio:.3e}")
    assert got.shape == (65, 4, 4) and ratio <= 1.0, (name, ratio)
    assert np.array_equal(got[tri < 0], np.zeros(((tri < 0).sum(), 4)))
    assert (got[tri >= 0][:, 3] > 0).any()
    # the defaults: the opaque grey ramp between the extremes of the values
    dflt = tc.shade(h, d, vals)
    assert np.array_equal(dflt[..., 3], (tri >= 0).astype(float))
    nanv = vals.copy()
    nanv[:] = np.nan
    assert not tc.shade(h, d, nanv, table, CLIM, AMBIENT).any(), "a non-finite value gives a zero layer"


def test_empty_soup_all_misses():
    with TriangleCaster(np.zeros((0, 3, 3))) as tc:
        h = tc.trace(np.zeros((3, 3)), np.ones((3, 3)), max_hits=2)
        assert (h.triangle == -1).all() and np.isinf(h.t).all() and np.isnan(h.u).all() and np.isnan(h.v).all()


# ---------------------------------------------------------------------------------------------------------------------
# layers in the volume
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ball():
    """The sphere soup in its 4 x 4 x 4 mesh, the 65 rays of the case, their samples on the twin and a smooth field."""
    geom = sphere_geom()
    pts, o, d, _, _, _ = case_soup("sphere")
    step = 0.13
    rays = rays_twin(clip_box_twin(geom), o, d, step)
    u = smooth(geom.xflat)[:, 0]
    vals = m.interpolate(geom, u, rays.pts)
    vals.setflags(write=False)
    return geom, pts, o, d, step, rays, u, vals


def test_render_with_all_miss_layers_is_bitwise_the_plain_render(ball):
    geom, pts, o, d, step, rays, u, vals = ball
    with RayCaster(geom, o, d, step) as rc:
        plain = rc.render(u, TABLE5, CLIM)
        for K in (1, 4):
            got = rc.render(u, TABLE5, CLIM, layers=(np.full((65, K), np.inf), np.zeros((65, K, 4))))
            assert np.array_equal(got, plain), K
        assert np.array_equal(rc.render(u, TABLE5, CLIM), plain), "the path without layers is unchanged afterwards"
        for layers, match in [
            ((np.full((65, 2), np.nan), np.zeros((65, 2, 4))), "must ascend"),
            ((np.tile([2.0, 1.0], (65, 1)), np.zeros((65, 2, 4))), "must ascend"),
            ((np.full((65, 1), np.inf), np.full((65, 1, 4), np.nan)), "must be finite"),
            ((np.full((64, 1), np.inf), np.zeros((64, 1, 4))), r"layers must be \(65, K\)"),
        ]:
            with pytest.raises(ValueError, match="RayCaster.render: .*" + match):
                rc.render(u, TABLE5, CLIM, layers=layers)


@pytest.mark.parametrize("K, alpha", [(1, 1.0), (4, 0.6)])
def test_render_with_layers_matches_the_twins_merge(ball, K, alpha):
    geom, pts, o, d, step, rays, u, vals = ball
    table = TABLE5.copy()
    table[:, 3] = alpha
    with TriangleCaster(pts) as tc:
        h = tc.trace(o, d, max_hits=K)
        layers = tc.shade(h, d, vertex_values(pts), table, CLIM, AMBIENT)
    assert (h.triangle >= 0).any() and sample_margin(rays, h.t) > MARGIN
    with RayCaster(geom, o, d, step) as rc:
        assert np.array_equal(rc.offsets, rays.offsets)
        got = rc.render(u, TABLE5, CLIM, layers=(h.t, layers))
        plain = rc.render(u, TABLE5, CLIM)
    want = composite_twin(rays, vals, TABLE5, *CLIM, h.t, layers)
    bound = 16 * (rays.n + 1 + K) * EPS * max(1.0, float(np.abs(TABLE5[:, :3]).max()))
    ratio = np.abs(got - want) / bound[:, None]
    record_observation(f"surface render layers K={K}: max difference / bound {ratio.max():.3e}")
    print(f"K = {K}: layered render max difference / bound {ratio.max():.3e}")
    assert (ratio <= 1.0).all(), (K, ratio.max())
    hit = h.triangle[:, 0] >= 0
    assert np.array_equal(got[~hit], plain[~hit]) and (got[hit] != plain[hit]).any()
    if alpha == 1.0:
        assert np.array_equal(got[hit, 3], np.ones(hit.sum())), "an opaque surface closes the ray"


# ---------------------------------------------------------------------------------------------------------------------
# render_surfaces, render_figure
# ---------------------------------------------------------------------------------------------------------------------

EYE, TARGET = (2.7, -3.1, 1.9), (0.0, 0.0, 0.0)


def test_render_figure_on_the_sphere():
    geom = sphere_geom()
    u = np.sum(geom.xflat ** 2, axis=1)
    W, H = 32, 24
    img = render_figure(geom, u, EYE, TARGET, size=(W, H), isosurfaces=[0.61], slices=[(0, 0.13)])
    assert img.shape == (H, W, 4) and img.dtype == np.float64 and np.isfinite(img).all()
    assert img[H // 2, W // 2, 3] == 1.0, "the opaque sphere closes the centre pixel"
    dflt = render_figure(geom, u, EYE, TARGET, size=(W, H))            # the reference's five isosurfaces
    assert dflt.shape == (H, W, 4) and np.isfinite(dflt).all() and dflt[H // 2, W // 2, 3] == 1.0
    glass = render_figure(geom, u, EYE, TARGET, size=(W, H), isosurfaces=[0.61], surface_alpha=0.5)
    assert np.isfinite(glass).all() and 0.0 < glass[H // 2, W // 2, 3] <= 1.0
    # the surfaces alone: alpha is 1 exactly where the brute force over the same soup reports a hit
    only = render_figure(geom, u, EYE, TARGET, size=(W, H), isosurfaces=[0.61], volume=False)
    soup = m.isocontour(geom, u, [0.61])
    o, d = camera_rays(EYE, TARGET, size=(W, H))
    tri = trace_twin(soup.points, o, d, 0.0, np.inf, 1)[1]
    assert only.shape == (H, W, 4) and np.isfinite(only).all()
    assert np.array_equal(only[..., 3], (tri[:, 0] >= 0).astype(float).reshape(H, W))
    assert 0 < (tri >= 0).sum() < W * H
    # render_surfaces on the same soup gives the same picture, and the depth of the first hit
    img2, depth = render_surfaces(soup, EYE, TARGET, size=(W, H), levels=[0.61], clim=(float(u.min()), float(u.max())),
                                  transfer=np.concatenate([m.raycast.default_transfer(1.0)[:, :3], np.ones((256, 1))], axis=1))
    assert np.array_equal(img2, only)
    assert np.array_equal(np.isfinite(depth), only[..., 3] == 1.0) and depth[H // 2, W // 2] > 3.0
    nothing = render_figure(geom, u, EYE, TARGET, size=(W, H), isosurfaces=[], volume=False)
    assert nothing.shape == (H, W, 4) and not nothing.any()
