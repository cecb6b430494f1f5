"""TriangleCaster / render_surfaces / render_figure on the CPU: every argument check raised before the library is
touched, the empty soup without a device, and the NumPy twin (tests/surface_twin.py) the GPU tests compare against,
itself pinned on exact answers.  The cases of tests/test_gpu_surface.py are defined here, so that the margin condition
their bitwise comparisons rely on is checked without a GPU, on the twin alone.
"""
import math

import numpy as np
import pytest

import mgb_amd as m
from contour_twin import isocontour_twin
from mgb_amd.raycast import RayCaster, camera_rays
from mgb_amd.surface import (Hits, TriangleCaster, composite_layers, default_surface_table, render_figure,
                             render_surfaces)
from raycast_twin import rays_twin
from surface_twin import (composite_twin, margin_twin, normalize_twin, pairs_twin, sample_margin, shade_twin,
                          trace_twin)
from test_raycast import CLIM, CUBE, EPS, TABLE5, centre_rays, closed_form, render_bound

MARGIN = 1e-9

# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_surface.py
# ---------------------------------------------------------------------------------------------------------------------

TRI = np.array([[0.21, 0.28, 0.52], [0.93, 0.37, 0.44], [0.38, 0.96, 0.61]])


def soup_one():
    return TRI[None].copy()


def soup_two():
    """Two triangles that share the edge v1-v2 of the first, bit for bit."""
    return np.stack([TRI, np.array([TRI[1], [0.97, 0.99, 0.38], TRI[2]])])


def soup_dup():
    """The same triangle twice, and one behind it."""
    return np.stack([TRI, TRI, TRI + np.array([0.05, -0.04, -0.3])])


def soup_random(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.1, 0.9, size=(n, 1, 3))
    return np.clip(c + 0.08 * rng.standard_normal((n, 3, 3)), 0.0, 1.0)


def soup_big():
    """One triangle across the whole box (registered in many cells) among 64 small ones."""
    big = np.array([[[-0.02, -0.03, 0.31], [1.04, 0.02, 0.47], [0.45, 1.05, 0.72]]])
    return np.concatenate([soup_random(32, 5), big, soup_random(32, 6)])


def soup_span():
    """One triangle across the whole unit box, then 64 small ones: the grid has many cells and the large triangle is in the
    lists of several cells along one ray, so a ray that keeps it meets it again in later cells."""
    big = np.array([[[-0.02, -0.03, 0.31], [1.04, 0.02, 0.47], [0.45, 1.05, 0.72]]])
    return np.concatenate([big, soup_random(64, 7)])


def sphere_geom():
    return m.subdivide(m.fem3d(k=1), 3)             # 4 x 4 x 4 elements


def soup_sphere():
    g = sphere_geom()
    return isocontour_twin(g, np.sum(g.xflat ** 2, axis=1), [0.61]).points


def soup_sphere_slices():
    g = sphere_geom()
    cuts = [isocontour_twin(g, g.xflat[:, a], [c]).points for a, c in ((0, 0.13), (1, -0.21), (2, 0.07))]
    return np.concatenate([soup_sphere()] + cuts)


def rays65(centre, scale):
    """65 rays around a soup of size `scale` at `centre`: a central ray first, pinhole rays (the corners of the image
    miss), axis-parallel rays with one and two zero components, rays that start inside, misses."""
    c = np.asarray(centre, dtype=np.float64)
    eye = c + scale * np.array([2.7, -3.1, 1.9])
    o, d = camera_rays(eye, c + scale * np.array([0.013, -0.021, 0.017]), size=(8, 6), fov=36.0)
    extra = [
        (eye, c + scale * np.array([0.031, 0.017, -0.023]) - eye),        # the central ray, first
        ((-3.0, 0.137, -0.211), (1.0, 0.0, 0.0)),                         # two zero components
        ((0.213, 5.0, 0.171), (0.0, -2.0, 0.0)),
        ((0.117, -0.193, -4.0), (0.0, 0.0, 1.0)),
        ((-3.0, 2.5, 0.043), (1.0, 0.0, 0.0)),                            # parallel to x, outside in y: misses
        ((-2.5, -2.2, 0.153), (1.0, 0.9, 0.0)),                           # one zero component
        ((0.231, -3.0, -2.0), (0.0, 1.0, 0.7)),
        ((5.0, 5.0, 5.0), (1.0, 0.2, 0.1)),                               # points away: misses
        ((-4.0, 0.019, 3.5), (1.0, 0.1, 0.0)),                            # passes above: misses
        ((0.113, -0.217, 0.319), (0.3, 0.5, -0.4)),                       # start inside
        ((0.023, 0.011, -0.017), (0.07, 0.03, 1.0)),
        ((-0.61, 0.67, -0.53), (-0.2, -1.0, 0.6)),
        ((0.41, 0.37, 0.29), (-1.0, -0.8, -0.55)),
        ((-0.17, 0.09, 0.05), (0.0, 0.31, -1.0)),
        ((0.3, -0.1, -0.2), (1.0, 0.0, 0.0)),
        ((0.05, 0.45, 0.1), (-0.4, -1.0, 0.3)),
        ((-0.33, -0.29, 0.47), (0.5, 0.45, -0.9)),
    ]
    eo = np.array([e[0] if i == 0 else c + scale * np.asarray(e[0]) for i, e in enumerate(extra)])
    ed = np.array([e[1] for e in extra], dtype=np.float64)
    o, d = np.concatenate([eo[:1], o, eo[1:]]), np.concatenate([ed[:1], d, ed[1:]])
    assert o.shape == (65, 3)
    return o, d


UNIT = ((0.5, 0.5, 0.5), 0.5)
BALL = ((0.0, 0.0, 0.0), 1.0)
# name -> (soup, (centre, scale) of the rays, t_min, t_max, excluded from the margin condition)
GPU_CASES = {
    "one": (soup_one, UNIT, 0.02, 2.35, False),
    "two": (soup_two, UNIT, 0.02, 2.35, False),
    "dup": (soup_dup, UNIT, 0.02, 2.35, True),
    "random256": (lambda: soup_random(256, 1), UNIT, 0.02, 2.35, False),
    "random257": (lambda: soup_random(257, 2), UNIT, 0.02, 2.35, False),
    "big": (soup_big, UNIT, 0.02, 2.35, False),
    "sphere": (soup_sphere, BALL, 0.05, 5.25, False),
    "sphere_slices": (soup_sphere_slices, BALL, 0.05, 5.25, False),
}
NRAYS = (1, 64, 65)
HITS = (1, 4, 8)


def case_soup(name):
    make, (centre, scale), t_min, t_max, tie = GPU_CASES[name]
    o, d = rays65(centre, scale)
    return make(), o, d, t_min, t_max, tie


def vertex_values(points):
    """(T, 3): a smooth function of the vertices."""
    P = points
    return np.sin(1.3 * P[..., 0] + 0.4) * np.cos(0.9 * P[..., 1] - 0.2) + 0.35 * np.sin(1.1 * P[..., 2] + 0.3)


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_gpu_cases_meet_the_margin_condition_on_the_twin(name):
    pts, o, d, t_min, t_max, tie = case_soup(name)
    t, tri, u, v, pr = trace_twin(pts, o, d, t_min, t_max, 8)
    margin, gap = margin_twin(pr, t_min, t_max)
    nh = pr.hit.sum(axis=1)
    print(f"{name}: T = {pts.shape[0]}, rays hit {int((nh > 0).sum())}/65, most hits {int(nh.max())}, margin "
          f"{margin:.3e}, gap {gap:.3e}")
    assert np.isfinite(pts).all()
    if tie:
        assert gap == 0.0, "the duplicate case has ties in t"
        return
    assert margin > MARGIN and gap > MARGIN
    dn = normalize_twin(d)
    # the mix every case is meant to have
    assert nh[0] > 0, "the first ray (the 1-ray bundle) hits"
    assert (nh > 0).sum() >= 3 and (nh == 0).any(), "hits and misses"
    zeros = (dn == 0.0).sum(axis=1)
    assert (zeros == 1).any() and (zeros == 2).any(), "axis-parallel rays with one and two zero components"
    with np.errstate(invalid="ignore"):
        inside = pr.ok & (pr.u >= 0) & (pr.v >= 0) & (pr.u + pr.v <= 1)
    cut_lo = (inside & (pr.t < t_min) & (pr.t > 0)).any()
    cut_hi = (inside & (pr.t > t_max)).any()
    if name != "one":
        assert cut_lo or cut_hi, "a hit that t_min or t_max cuts off"


def test_span_soup_keeps_its_large_triangle_on_the_twin():
    """What test_gpu_surface.py's test of a triangle met in several cells relies on, from the twin alone: the margin
    condition of a bitwise comparison, and rays that keep the large triangle (index 0) for K = 1 and K = 8."""
    pts = soup_span()
    o, d = rays65(*UNIT)
    t, tri, u, v, pr = trace_twin(pts, o, d, 0.02, 2.35, 8)
    margin, gap = margin_twin(pr, 0.02, 2.35)
    first, kept = int((tri[:, 0] == 0).sum()), int((tri == 0).any(axis=1).sum())
    print(f"span: margin {margin:.3e}, gap {gap:.3e}; the large triangle is the nearest hit of {first} rays and among the "
          f"8 nearest of {kept}")
    assert margin > MARGIN and gap > MARGIN
    assert first >= 1 and kept > first, "kept as the nearest hit (K = 1) and behind others (K = 8)"
    ext = pts[0].max(axis=0) - pts[0].min(axis=0)
    assert (ext[:2] > 1.0).all() and (pts[1:].max(axis=1) - pts[1:].min(axis=1)).max() < 0.7


def test_large_cases_have_rays_with_many_hits():
    for name in ("sphere", "sphere_slices", "random257"):
        pts, o, d, t_min, t_max, _ = case_soup(name)
        pr = pairs_twin(pts, o, normalize_twin(d), t_min, t_max)
        assert pr.hit.sum(axis=1).max() >= 2, name
    pts, o, d, t_min, t_max, _ = case_soup("sphere_slices")
    assert pairs_twin(pts, o, normalize_twin(d), t_min, t_max).hit.sum(axis=1).max() > 4, "K = 4 truncates a ray"


def test_no_hit_of_the_layered_render_case_is_at_a_sample():
    """tests/test_gpu_surface.py merges the hits of the sphere case into the samples of step 0.13 through its mesh."""
    from raycast_twin import clip_box_twin
    pts, o, d, _, _, _ = case_soup("sphere")
    rays = rays_twin(clip_box_twin(sphere_geom()), o, d, 0.13)
    t = trace_twin(pts, o, d, 0.0, math.inf, 4)[0]
    assert np.isfinite(t).any() and (rays.n > 0).any() and sample_margin(rays, t) > MARGIN
    assert rays.half_integer_margin() > 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# the twin on exact answers
# ---------------------------------------------------------------------------------------------------------------------

UNIT_TRI = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])


def test_twin_unit_triangle_axis_rays():
    o = np.array([[0.25, 0.5, 3.0], [0.125, 0.25, -2.0], [0.75, 0.5, 1.0], [0.3, 0.3, 1.0]])
    d = np.array([[0.0, 0.0, -2.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0]])
    t, tri, u, v, _ = trace_twin(UNIT_TRI, o, d, 0.0, math.inf, 1)
    assert tri[:, 0].tolist() == [0, 0, -1, -1]             # outside u + v <= 1; pointing away
    for r, (tt, uu, vv) in enumerate([(3.0, 0.25, 0.5), (2.0, 0.125, 0.25)]):
        assert abs(t[r, 0] - tt) <= 4 * EPS * tt and abs(u[r, 0] - uu) <= 4 * EPS and abs(v[r, 0] - vv) <= 4 * EPS
    assert np.isinf(t[2:, 0]).all() and np.isnan(u[2:, 0]).all() and np.isnan(v[2:, 0]).all()
    # two-sided, and t_min / t_max are inclusive bounds
    assert trace_twin(UNIT_TRI, o[:1], d[:1], 3.0, 3.0 + 1e-9, 1)[1][0, 0] == 0
    assert trace_twin(UNIT_TRI, o[:1], d[:1], 3.0 + 1e-9, 9.0, 1)[1][0, 0] == -1
    assert trace_twin(UNIT_TRI, o[:1], d[:1], 0.0, 3.0 - 1e-9, 1)[1][0, 0] == -1


def test_twin_duplicate_triangle_tie_goes_to_the_lower_index():
    pts = np.concatenate([UNIT_TRI, UNIT_TRI, UNIT_TRI])
    t, tri, u, v, _ = trace_twin(pts, [[0.25, 0.25, 1.0]], [[0.0, 0.0, -1.0]], 0.0, math.inf, 2)
    assert tri.tolist() == [[0, 1]] and t[0, 0] == t[0, 1] == 1.0


def test_twin_shared_edge_is_hit_lower_index_first():
    a, b = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 0.0])
    pts = np.array([[a, [1.0, 0.0, 0.0], b], [a, b, [0.0, 1.0, 0.0]]])
    t, tri, u, v, _ = trace_twin(pts, [[0.5, 0.5, 2.0]], [[0.0, 0.0, -1.0]], 0.0, math.inf, 2)
    assert tri.tolist() == [[0, 1]] and t.tolist() == [[2.0, 2.0]]


def test_twin_degenerate_triangle_is_never_hit():
    pts = np.array([[[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [2.0, 2.0, 0.0]], [[0.3, 0.3, 0.0]] * 3])
    o = np.array([[0.5, 0.5, 1.0], [0.3, 0.3, 1.0], [1.0, 1.0, 1.0]])
    d = np.tile([0.0, 0.0, -1.0], (3, 1))
    t, tri, _, _, pr = trace_twin(pts, o, d, 0.0, math.inf, 2)
    assert (tri == -1).all() and not pr.ok.any()


def test_twin_stack_of_ten_keeps_the_nearest_four_in_order():
    z = np.array([0.7, 0.1, 0.9, 0.3, 1.0, 0.2, 0.8, 0.4, 0.6, 0.5])
    pts = np.stack([UNIT_TRI[0] + np.array([0.0, 0.0, zz]) for zz in z])
    t, tri, _, _, _ = trace_twin(pts, [[0.25, 0.25, 2.0]], [[0.0, 0.0, -3.0]], 0.0, math.inf, 4)
    assert tri.tolist() == [[4, 2, 6, 0]]                   # z = 1.0, 0.9, 0.8, 0.7 seen from above
    assert np.abs(t[0] - (2.0 - z[[4, 2, 6, 0]])).max() <= 4 * EPS * 2.0


def test_twin_opaque_layer_in_a_constant_volume_is_the_closed_form():
    o, d, chord = centre_rays()
    rays = rays_twin(CUBE, o, d, 0.13)
    R = rays.n.size
    mcut = np.maximum(1, rays.n // 3)
    t_star = rays.tmin + mcut * rays.h                      # between samples mcut - 1 and mcut
    assert sample_margin(rays, t_star[:, None]) > 1e-3
    layer = np.tile([0.3, 0.6, 0.2, 1.0], (R, 1, 1))
    for c in (0.31, -0.9, 2.0):
        got = composite_twin(rays, np.full(rays.pts.shape[0], c), TABLE5, *CLIM, t_star[:, None], layer)
        vol = closed_form(TABLE5, CLIM, c, mcut * rays.h)
        want = np.concatenate([vol[:, :3] + (1.0 - vol[:, 3:]) * layer[:, 0, :3], np.ones((R, 1))], axis=1)
        assert (np.abs(got - want) <= render_bound(rays.n, TABLE5)[:, None]).all(), c
    # without hits the merge is the plain composite; a hit behind the last sample is applied after it
    from raycast_twin import render_twin
    vals = np.full(rays.pts.shape[0], 0.31)
    none = composite_twin(rays, vals, TABLE5, *CLIM, np.full((R, 2), np.inf), np.zeros((R, 2, 4)))
    assert np.array_equal(none, render_twin(rays, vals, TABLE5, *CLIM))
    behind = composite_twin(rays, vals, TABLE5, *CLIM, (rays.tmin + rays.chord + 1.0)[:, None], layer)
    assert np.array_equal(behind[:, 3], np.ones(R))
    assert np.abs(behind[:, :3] - (none[:, :3] + (1.0 - none[:, 3:]) * layer[:, 0, :3])).max() <= 8 * EPS


def test_twin_shade_formula():
    dn = normalize_twin(np.array([[0.0, 0.0, -1.0], [0.0, 3.0, -4.0]]))
    tri = np.array([[0], [0]], dtype=np.int32)
    u, v = np.array([[0.25], [0.5]]), np.array([[0.5], [0.25]])
    vals = np.array([[0.0, 1.0, 2.0]])
    table = np.array([[0.0, 0.0, 1.0, 0.5], [1.0, 0.5, 0.0, 1.5]])
    L = shade_twin(UNIT_TRI, dn, tri, u, v, vals, table, 0.0, 2.0, 0.3)
    for r, (c, cosv) in enumerate([(1.25, 1.0), (1.0, 0.8)]):
        w = c / 2.0
        alpha = min(1.0, 0.5 + w)
        shade = 0.3 + 0.7 * cosv
        want = [alpha * shade * w, alpha * shade * 0.5 * w, alpha * shade * (1.0 - w), alpha]
        assert np.abs(L[r, 0] - want).max() <= 8 * EPS
    missing = shade_twin(UNIT_TRI, dn, np.array([[-1], [0]], dtype=np.int32), u, v, np.array([[0.0, np.nan, 2.0]]),
                         table, 0.0, 2.0, 0.3)
    assert np.array_equal(missing, np.zeros((2, 1, 4)))     # a missing hit, a non-finite value


def test_composite_layers_is_the_twins_merge_without_samples():
    rng = np.random.default_rng(3)
    layers = rng.uniform(0.0, 1.0, size=(5, 3, 4))
    rays = rays_twin(CUBE, np.full((5, 3), 9.0), np.ones((5, 3)), 0.1)       # all miss: no samples
    want = composite_twin(rays, np.zeros(0), TABLE5, *CLIM, np.tile([1.0, 2.0, 3.0], (5, 1)), layers)
    assert np.abs(composite_layers(layers) - want).max() <= 4 * EPS


# ---------------------------------------------------------------------------------------------------------------------
# the empty soup and every refusal, without a device
# ---------------------------------------------------------------------------------------------------------------------

O2, D2 = np.zeros((2, 3)), np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 1.0]])


def test_names_are_exported():
    assert m.TriangleCaster is TriangleCaster and m.render_surfaces is render_surfaces
    assert m.render_figure is render_figure and m.Hits is Hits
    T = default_surface_table()
    assert T.shape == (256, 4) and np.array_equal(T[:, 3], np.ones(256)) and np.array_equal(T[:, 0], np.arange(256) / 255)


def test_empty_soup_misses_without_a_device():
    with TriangleCaster(np.zeros((0, 3, 3))) as tc:
        h = tc.trace(O2, D2, max_hits=3)
        assert h.t.shape == (2, 3) and np.isinf(h.t).all() and (h.triangle == -1).all() and h.triangle.dtype == np.int32
        assert np.isnan(h.u).all() and np.isnan(h.v).all()
        assert np.array_equal(tc.shade(h, D2, np.zeros((0, 3))), np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="TriangleCaster: the caster is closed"):
        tc.trace(O2, D2)
    empty = m.Contour(np.zeros((0, 3, 3)), np.zeros(0, np.int32), np.zeros(0, np.int32), None, 1)
    img, depth = render_surfaces(empty, (3, 2, 1), (0, 0, 0), size=(4, 3), levels=[0.5])
    assert img.shape == (3, 4, 4) and not img.any() and depth.shape == (3, 4) and np.isinf(depth).all()


@pytest.mark.parametrize("points, match", [
    (np.zeros((2, 3)), r"points must be \(T, 3, 3\)"),
    (np.zeros((2, 3, 2)), r"points must be \(T, 3, 3\)"),
    (np.full((1, 3, 3), np.nan), "every entry of points must be finite"),
    (np.full((1, 3, 3), np.inf), "every entry of points must be finite"),
])
def test_points_refusals(points, match):
    with pytest.raises(ValueError, match="TriangleCaster: .*" + match):
        TriangleCaster(points)


@pytest.mark.parametrize("kw, match", [
    (dict(o=np.zeros((2, 2))), r"o and d must both be \(R, 3\)"),
    (dict(d=np.ones((3, 3))), r"o and d must both be \(R, 3\)"),
    (dict(o=np.array([[np.nan, 0, 0], [0, 0, 0]])), "every ray origin o must be finite"),
    (dict(d=np.array([[np.inf, 0, 0], [0, 1, 0]])), "every ray direction d must be finite"),
    (dict(d=np.array([[0.0, 0, 0], [0, 1, 0]])), "a ray direction d is zero"),
    (dict(d=np.array([[1e200, 1e200, 0], [0, 1, 0]])), "too long or too short to normalise"),
    (dict(max_hits=0), r"max_hits must be an integer in 1\.\.8"),
    (dict(max_hits=9), r"max_hits must be an integer in 1\.\.8"),
    (dict(max_hits=True), r"max_hits must be an integer in 1\.\.8"),
    (dict(max_hits=2.0), r"max_hits must be an integer in 1\.\.8"),
    (dict(t_min=1.0, t_max=1.0), "t_max must be greater than t_min"),
    (dict(t_min=2.0, t_max=1.0), "t_max must be greater than t_min"),
    (dict(t_min=-np.inf), "t_min must be finite"),
    (dict(t_max=np.nan), "t_max must be greater than t_min"),
    (dict(t_min="a"), "t_min and t_max must be numbers"),
])
def test_trace_refusals(kw, match):
    args = dict(o=O2, d=D2)
    args.update(kw)
    with TriangleCaster(np.zeros((0, 3, 3))) as tc:
        with pytest.raises(ValueError, match="TriangleCaster.trace: .*" + match):
            tc.trace(**args)


def test_shade_refusals():
    with TriangleCaster(np.zeros((0, 3, 3))) as tc:
        h = tc.trace(O2, D2, max_hits=2)
        V = np.zeros((0, 3))
        for args, kw, match in [
            (((h.t, h.triangle), D2, V), {}, "hits must be what trace"),
            ((h, D2[:1], V), {}, "hits hold"),
            ((h, np.zeros((2, 3)), V), {}, "a ray direction d is zero"),
            ((h, D2, np.zeros((1, 3))), {}, r"values must be \(0, 3\)"),
            ((h, D2, np.zeros(3)), {}, r"values must be \(0, 3\)"),
            ((Hits(h.t, np.zeros((2, 2), np.int32), h.u, h.v), D2, V), {}, r"an index outside -1\.\.-1"),
            ((Hits(h.t, h.triangle, h.u[:, :1], h.v), D2, V), {}, "hits.u and hits.v must have the shape"),
            ((h, D2, V), dict(transfer=np.zeros((1, 4))), r"transfer must be \(K, 4\) with K >= 2"),
            ((h, D2, V), dict(transfer=np.full((3, 4), np.nan)), "every transfer entry must be finite"),
            ((h, D2, V), dict(clim=(1.0, 1.0)), "clim must be finite with lo < hi"),
            ((h, D2, V), dict(clim=3.0), r"clim must be \(lo, hi\)"),
            ((h, D2, V), dict(ambient=1.5), r"ambient must be a number in \[0, 1\]"),
            ((h, D2, V), dict(ambient=np.nan), r"ambient must be a number in \[0, 1\]"),
        ]:
            with pytest.raises(ValueError, match="TriangleCaster.shade: .*" + match):
                tc.shade(*args, **kw)


def test_render_surfaces_refusals():
    tri = m.Contour(UNIT_TRI.copy(), np.zeros(1, np.int32), np.zeros(1, np.int32), None, 1)
    seg = m.Contour(np.zeros((1, 2, 2)), np.zeros(1, np.int32), np.zeros(1, np.int32), None, 1)
    cam = dict(eye=(3, 2, 1), target=(0, 0, 0), size=(4, 3))
    for contours, kw, match in [
        (UNIT_TRI, {}, "contours must be a Contour or a list of them"),
        ([tri, 3], {}, "contours must be a Contour or a list of them"),
        (seg, {}, "contours must hold triangles"),
        (tri, {}, "needs values= or levels="),
        (tri, dict(values=np.zeros(2)), r"values must be \(1,\) or \(1, 3\)"),
        (tri, dict(levels=[0.1, 0.2]), r"levels\[0\] has 2 values for a contour of 1 levels"),
        ([tri, tri], dict(levels=[[0.1]]), "one array of level values per contour"),
        (tri, dict(values=np.ones(1), max_hits=0), r"max_hits must be an integer in 1\.\.8"),
        (tri, dict(values=np.ones(1), ambient=-0.1), "ambient must be a number"),
        (tri, dict(values=np.ones(1), transfer=np.zeros((2, 3))), r"transfer must be \(K, 4\)"),
        (tri, dict(values=np.ones(1)), "values is constant"),
        (tri, dict(values=np.full(1, np.nan)), "values has no finite entry"),
    ]:
        with pytest.raises(ValueError, match="render_surfaces: .*" + match):
            render_surfaces(contours, **cam, **kw)
    with pytest.raises(ValueError, match="camera_rays: size"):
        render_surfaces(tri, (3, 2, 1), (0, 0, 0), size=(0, 3), values=np.ones(1))


def test_render_figure_refusals():
    g3 = m.fem3d(k=1)
    u = g3.xflat @ np.array([1.0, 2.0, 4.0])
    cam = dict(eye=(3, 2, 1), target=(0, 0, 0), size=(4, 3))
    g2 = m.fem2d(k=1)
    with pytest.raises(ValueError, match="render_figure: fem2d geometries are not supported"):
        render_figure(g2, np.zeros(g2.xflat.shape[0]), **cam)
    with pytest.raises(ValueError, match="render_figure: fem1d geometries are not supported"):
        render_figure(m.fem1d(), np.zeros(4), **cam)
    for uu, kw, match in [
        (u[:-1], {}, "u must be a vector of"),
        (np.ones_like(u), {}, r"render_figure: u is constant"),
        (u, dict(clim=(2.0, 1.0)), "clim must be finite with lo < hi"),
        (u, dict(isosurfaces=[0.5, np.nan]), "every entry of isosurfaces must be finite"),
        (u, dict(slices=[(3, 0.1)]), "a slice needs an axis in 0..2"),
        (u, dict(slices=[(0, np.inf)]), "a slice needs an axis in 0..2"),
        (u, dict(slices=[0.3]), r"slices must be a list of \(axis, coordinate\) pairs"),
        (u, dict(surface_alpha=1.2), r"surface_alpha must be a number in \[0, 1\]"),
        (u, dict(ambient=2), "ambient must be a number"),
        (u, dict(step=0.0), "step must be finite and positive"),
        (u, dict(transfer=np.zeros((2, 3))), r"transfer must be \(K, 4\)"),
    ]:
        with pytest.raises(ValueError, match=match):
            render_figure(g3, uu, **cam, **kw)
    with pytest.raises(ValueError, match="camera_rays: eye and target coincide"):
        render_figure(g3, u, (0, 0, 0), (0, 0, 0))


def test_render_layers_refusals():
    g3 = m.fem3d(k=1)
    u = g3.xflat @ np.array([1.0, 2.0, 4.0])
    with RayCaster(g3, np.zeros((0, 3)), np.zeros((0, 3)), 0.1) as rc:
        assert rc.render(u, layers=(np.zeros((0, 2)), np.zeros((0, 2, 4)))).shape == (0, 4)
        for layers, match in [
            (np.zeros((0, 2)), r"layers must be \(t_hit, layer\)"),
            ((np.zeros((0, 9)), np.zeros((0, 9, 4))), r"with K in 1\.\.8"),
            ((np.zeros((0, 2)), np.zeros((0, 2, 3))), r"with K in 1\.\.8"),
            ((np.zeros((1, 2)), np.zeros((1, 2, 4))), r"layers must be \(0, K\)"),
        ]:
            with pytest.raises(ValueError, match="RayCaster.render: .*" + match):
                rc.render(u, layers=layers)
    g2 = m.fem2d(k=1)
    with RayCaster(g2, np.zeros((0, 2)), np.zeros((0, 2)), 0.1) as rc:
        with pytest.raises(ValueError, match="RayCaster.render: layers need a 3-D mesh"):
            rc.render(np.arange(4.0), layers=(np.zeros((0, 1)), np.zeros((0, 1, 4))))
