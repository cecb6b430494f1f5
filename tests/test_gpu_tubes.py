"""SegmentCaster / render_lines / render_curve / render_figure(lines=...) on the device against the NumPy twin
(tests/tubes_twin.py), which tests every ray against every capsule without a grid.

Both sides run the same IEEE additions and products in the same order without contraction; only the square roots and
the divisions may round differently, by at most one ulp each.  So once no pair sits within 1e-9 of a decision (asserted
on the twin alone in tests/test_tubes.py, where the cases live) the segments and the winning pieces are compared
exactly, `t` within `4 eps (|t| + sqrt(h) / A)` on the side and `4 eps (|t| + sqrt(h2))` on a cap, `s` within
`(|bard| bound_t + 2 eps (|baoa| + |t bard|)) / baba + eps |s|` on the side and exactly on the caps
(`tubes_twin.t_bound`, `s_bound`).  `shade` is given the device's own hits on both sides: 16 eps max(1, max|table
colour|) per channel.  The composed pictures are bitwise, because the same device calls run on both sides.
"""
import numpy as np
import pytest

import mgb_amd as m
from helpers import record_observation
from mgb_amd.raycast import RayCaster, camera_rays, clip_box, default_transfer, _diagonal
from mgb_amd.surface import TriangleCaster, composite_layers, render_figure
from mgb_amd.tubes import SegmentCaster, curve_segments, merge_layers, render_curve, render_lines, segments
from test_manifold_post import sphere
from test_raycast import CLIM, TABLE5
from test_tubes import GPU_CASES, HITS, NRAYS, TIES, case_tubes, circle3, dup_segments, end_values
from tubes_twin import EPS, normalize_twin, piece_of, s_bound, shade_twin, t_bound, trace_twin

pytestmark = pytest.mark.gpu

AMBIENT = 0.3


@pytest.fixture(params=sorted(set(GPU_CASES) - set(TIES)), scope="module")
def case(request):
    """One caster per case, shared by its tests, with the twin's hits for K = 8 (computed once, never modified)."""
    name = request.param
    pts, rad, o, d, t_min, t_max = case_tubes(name)
    twin = trace_twin(pts, rad, o, d, t_min, t_max, 8)
    worst = {"t": 0.0, "s": 0.0}
    with SegmentCaster(pts, rad) as sc:
        yield name, pts, o, d, t_min, t_max, twin, sc, worst
    record_observation(f"tubes trace {name}: max error / bound, t {worst['t']:.3e}, s {worst['s']:.3e}")
    print(f"{name}: trace max error / bound, t {worst['t']:.3e}, s {worst['s']:.3e}")


@pytest.mark.parametrize("K", HITS)
@pytest.mark.parametrize("R", NRAYS)
def test_trace_matches_the_twin(case, R, K):
    name, pts, o, d, t_min, t_max, twin, sc, worst = case
    h = sc.trace(o[:R], d[:R], t_min, t_max, max_hits=K)
    t, seg, s, piece = (a[:R, :K] for a in (twin.t, twin.segment, twin.s, twin.piece))     # the first K of the 8 nearest
    bt, bs = t_bound(twin)[:R, :K], s_bound(twin)[:R, :K]
    assert h.segment.dtype == np.int32 and h.segment.shape == (R, K) and h.t.dtype == np.float64 and h.s.shape == (R, K)
    assert np.array_equal(h.segment, seg), (name, R, K)
    assert np.array_equal(piece_of(h.s, h.segment), piece), (name, R, K)
    hit = seg >= 0
    assert np.isinf(h.t[~hit]).all() and (h.t[~hit] > 0).all() and np.isnan(h.s[~hit]).all()
    if hit.any():
        rt = float((np.abs(h.t[hit] - t[hit]) / bt[hit]).max())
        side = hit & (bs > 0)
        rs = float((np.abs(h.s[side] - s[side]) / bs[side]).max()) if side.any() else 0.0
        print(f"{name} R = {R} K = {K}: max error / bound, t {rt:.3e}, s {rs:.3e}")
        worst["t"], worst["s"] = max(worst["t"], rt), max(worst["s"], rs)
        assert rt <= 1.0 and rs <= 1.0, (name, R, K, rt, rs)
        assert np.array_equal(h.s[hit & ~side], s[hit & ~side]), "s is 0 or 1 exactly on the caps"
    again = sc.trace(o[:R], d[:R], t_min, t_max, max_hits=K)
    for a, b in ((h.t, again.t), (h.segment, again.segment), (h.s, again.s)):
        assert np.array_equal(a, b, equal_nan=True), "two trace calls are bitwise equal"


@pytest.fixture(params=["dup", "helix"], scope="module")
def dispatch_case(request):
    name = request.param
    pts, rad, o, d, t_min, t_max = case_tubes(name)
    twin = trace_twin(pts, rad, o, d, t_min, t_max, 8)
    with SegmentCaster(pts, rad) as sc:
        yield name, o, d, t_min, t_max, twin, sc


@pytest.mark.parametrize("K", range(1, 9))
def test_every_hit_count_matches_the_twin(dispatch_case, K):
    """Every case of the one dispatch over the hit count, at one full wave plus one lane, with the bounds of
    test_trace_matches_the_twin."""
    name, o, d, t_min, t_max, twin, sc = dispatch_case
    h = sc.trace(o, d, t_min, t_max, max_hits=K)
    t, seg, s, piece = (a[:, :K] for a in (twin.t, twin.segment, twin.s, twin.piece))      # the first K of the 8 nearest
    bt, bs = t_bound(twin)[:, :K], s_bound(twin)[:, :K]
    assert h.segment.shape == (65, K) and np.array_equal(h.segment, seg), (name, K)
    assert np.array_equal(piece_of(h.s, h.segment), piece), (name, K)
    hit = seg >= 0
    assert hit.any() and np.isinf(h.t[~hit]).all() and (h.t[~hit] > 0).all() and np.isnan(h.s[~hit]).all()
    side = hit & (bs > 0)
    rt = float((np.abs(h.t[hit] - t[hit]) / bt[hit]).max())
    rs = float((np.abs(h.s[side] - s[side]) / bs[side]).max()) if side.any() else 0.0
    print(f"{name} K = {K}: max error / bound, t {rt:.3e}, s {rs:.3e}")
    assert rt <= 1.0 and rs <= 1.0, (name, K, rt, rs)
    assert np.array_equal(h.s[hit & ~side], s[hit & ~side]), "s is 0 or 1 exactly on the caps"


def test_ties_go_to_the_lower_index():
    """The deliberate tie, outside the margin condition: a duplicated segment.  Both are reported, the lower index
    first, with equal t."""
    pts, rad, o, d, t_min, t_max = case_tubes("dup")
    tw = trace_twin(pts, rad, o, d, t_min, t_max, 3)
    with SegmentCaster(pts, rad) as sc:
        h = sc.trace(o, d, t_min, t_max, max_hits=3)
    assert np.array_equal(h.segment, tw.segment) and np.array_equal(piece_of(h.s, h.segment), tw.piece)
    hit = tw.segment >= 0
    assert (np.abs(h.t[hit] - tw.t[hit]) <= t_bound(tw)[hit]).all()
    tie = (h.segment[:, 1] >= 0) & (h.t[:, 0] == h.t[:, 1])
    assert tie.any() and np.array_equal(h.segment[tie][:, :2], np.tile([0, 1], (tie.sum(), 1)))
    assert np.array_equal(h.s[tie, 0], h.s[tie, 1])


def test_shade_matches_the_twin(case):
    name, pts, o, d, t_min, t_max, twin, sc, _ = case
    h = sc.trace(o, d, t_min, t_max, max_hits=4)
    vals = end_values(pts)
    table = TABLE5.copy()
    table[:, 3] = [0.0, 0.7, 1.3, 0.4, 1.0]                # alphas on both sides of the clamp
    got = sc.shade(h, o, d, vals, table, CLIM, AMBIENT)
    want = shade_twin(pts, o, normalize_twin(d), h.t, h.segment, h.s, vals, table, *CLIM, AMBIENT)   # the device's own hits
    bound = 16 * EPS * max(1.0, float(np.abs(table[:, :3]).max()))
    ratio = float(np.abs(got - want).max() / bound)
    record_observation(f"tubes shade {name}: max difference / bound {ratio:.3e}")
    print(f"{name}: shade max difference / bound {ratio:.3e}")
    miss = h.segment < 0
    assert got.shape == (65, 4, 4) and ratio <= 1.0, (name, ratio)
    assert np.array_equal(got[miss], np.zeros((miss.sum(), 4))), "missing hits give zero layers exactly"
    assert (got[~miss][:, 3] > 0).any()
    if float(vals.min()) < float(vals.max()):               # the defaults: the opaque grey ramp between the extremes
        dflt = sc.shade(h, o, d, vals)
        assert np.array_equal(dflt[..., 3], (~miss).astype(float))
    else:                                                   # one sphere: both end values are one number
        with pytest.raises(ValueError, match="SegmentCaster.shade: values is constant"):
            sc.shade(h, o, d, vals)
    nanv = np.full_like(vals, np.nan)
    assert not sc.shade(h, o, d, nanv, table, CLIM, AMBIENT).any(), "a non-finite value gives a zero layer"


def test_empty_soup_all_misses():
    with SegmentCaster(np.zeros((0, 2, 3)), 0.1) as sc:
        h = sc.trace(np.zeros((3, 3)), np.ones((3, 3)), max_hits=2)
        assert (h.segment == -1).all() and np.isinf(h.t).all() and np.isnan(h.s).all()
        assert not sc.shade(h, np.zeros((3, 3)), np.ones((3, 3)), np.zeros((0, 2))).any()


# ---------------------------------------------------------------------------------------------------------------------
# composition by parts: bitwise, the same device calls on both sides
# ---------------------------------------------------------------------------------------------------------------------

EYE, TARGET = (2.7, -3.1, 1.9), (0.0, 0.0, 0.0)
W, H = 32, 24
COLOR = (0.9, 0.1, 0.2)


def line_layers(pts, o, d, radius, color=COLOR):
    table = np.tile(np.concatenate([color, [1.0]]), (2, 1))
    with SegmentCaster(pts, radius) as sc:
        lh = sc.trace(o, d, max_hits=1)
        return lh.t, sc.shade(lh, o, d, np.zeros((pts.shape[0], 2)), table, (0.0, 1.0), AMBIENT)


@pytest.fixture(scope="module")
def cube():
    """fem3d k = 1 subdivided twice, a smooth field and its gradient lines from 5 seeds, 20 steps."""
    geom = m.subdivide(m.fem3d(k=1), 2)
    x = geom.xflat
    u = np.sin(1.1 * x[:, 0] + 0.3) + 0.8 * np.cos(0.9 * x[:, 1] - 0.2) + 0.6 * x[:, 2] + 0.25 * x[:, 0] * x[:, 2]
    seeds = np.array([[-0.6, -0.5, -0.4], [0.1, -0.3, 0.2], [0.4, 0.5, -0.6], [-0.2, 0.6, 0.3], [0.0, 0.0, 0.0]])
    st = m.streamlines(geom, u, seeds, step=0.05, max_steps=20, field="gradient")
    assert (st.n >= 2).all()
    return geom, u, st


@pytest.mark.parametrize("volume", [True, False])
def test_render_figure_with_streamlines_is_the_hand_composition(cube, volume):
    geom, u, st = cube
    lev = 0.5 * (float(u.min()) + float(u.max()))
    kw = dict(size=(W, H), isosurfaces=[lev], volume=volume)
    got = render_figure(geom, u, EYE, TARGET, lines=st, line_color=COLOR, **kw)
    o, d = camera_rays(EYE, TARGET, size=(W, H))
    diag = _diagonal(clip_box(geom))
    clim = (float(u.min()), float(u.max()))
    table = default_transfer(diag)
    surf = table.copy()
    surf[:, 3] = 1.0
    iso = m.isocontour(geom, u, [lev])
    with TriangleCaster(iso.points) as tc:
        hits = tc.trace(o, d, max_hits=1)
        layers = tc.shade(hits, d, np.full((iso.points.shape[0], 3), lev), surf, clim, AMBIENT)
    pts, none = segments(st)
    assert none is None and pts.shape == (int((st.n - 1).sum()), 2, 3)
    lt, ll = line_layers(pts, o, d, 0.01 * diag)
    t, lay = merge_layers((hits.t, layers), (lt, ll), max_hits=8)
    if volume:
        with RayCaster(geom, o, d, diag / 256.0) as rc:
            want = rc.render(u, table, clim, layers=(t, lay))
    else:
        want = composite_layers(lay)
    assert got.shape == (H, W, 4) and np.array_equal(got, want.reshape(H, W, 4))
    plain = render_figure(geom, u, EYE, TARGET, **kw)
    assert (got != plain).any(), "the lines show"
    assert np.isfinite(lt).any() and (np.isfinite(lt[:, 0]) & ~(hits.t[:, 0] < lt[:, 0])).any(), "a line in front"
    # an explicit radius and the default colour (black) differ from both
    thick = render_figure(geom, u, EYE, TARGET, lines=st, line_radius=0.05, **kw)
    assert (thick != got).any() and (thick != plain).any()
    assert np.array_equal(render_figure(geom, u, EYE, TARGET, lines=[], **kw), plain), "no lines: today's image"


def test_render_figure_on_a_surface_draws_its_level_curves():
    gs = sphere(1, 1)
    us = np.sin(1.3 * gs.xflat[:, 0] + 0.4) + 0.7 * gs.xflat[:, 2]
    levels = [float(np.quantile(us, 0.35)), float(np.quantile(us, 0.7))]
    eye = (0.5, -4.0, 1.5)
    got = render_figure(gs, us, eye, TARGET, size=(W, H), lines=levels, line_color=COLOR)
    plain = render_figure(gs, us, eye, TARGET, size=(W, H))
    o, d = camera_rays(eye, TARGET, size=(W, H))
    clim = (float(us.min()), float(us.max()))
    surf = default_transfer(1.0)
    surf[:, 3] = 1.0
    tess = m.tessellate(gs, us)
    with TriangleCaster(tess.points) as tc:
        hits = tc.trace(o, d, max_hits=1)
        layers = tc.shade(hits, d, tess.values[..., 0], surf, clim, AMBIENT)
    assert np.array_equal(composite_layers(layers).reshape(H, W, 4), plain)
    con = m.isocontour(gs, us, levels)
    assert con.points.shape[1:] == (2, 3) and con.points.shape[0] > 0
    diag = _diagonal(np.stack([gs.xflat.min(axis=0), gs.xflat.max(axis=0)]))
    lt, ll = line_layers(con.points, o, d, 0.01 * diag)
    _, lay = merge_layers((hits.t, layers), (lt, ll), max_hits=8)
    assert np.array_equal(got, composite_layers(lay).reshape(H, W, 4))
    assert (got != plain).any(), "the level curves show"
    assert np.array_equal(render_figure(gs, us, eye, TARGET, size=(W, H), lines=con, line_color=COLOR), got)
    assert np.array_equal(render_figure(gs, us, eye, TARGET, size=(W, H), lines=[]), plain)


@pytest.mark.parametrize("e", [3, 2])
def test_render_curve_is_render_lines_of_its_segments(e):
    K = circle3(8, 2)
    geom = m.fem1d(k=2, K=K if e == 3 else K[..., :2], ambient=e)
    z = np.cos(2.0 * np.arctan2(geom.xflat[:, 1], geom.xflat[:, 0])) + 0.1 * geom.xflat[:, 0]
    eye = (2.5, -3.0, 2.2)
    kw = dict(size=(W, H), max_hits=2)
    img, depth = render_curve(geom, z, eye, TARGET, height_scale=0.5, **kw)
    pts, vals = curve_segments(geom, z, height_scale=0.5)
    img2, depth2 = render_lines(pts, eye, TARGET, values=vals, **kw)
    assert img.shape == (H, W, 4) and np.array_equal(img, img2) and np.array_equal(depth, depth2)
    assert img.any() and np.isfinite(depth).any() and np.isinf(depth).any() and np.isfinite(img).all()
    assert np.array_equal(np.isfinite(depth), img[..., 3] > 0), "the default table is opaque"
    # by hand: the default radius, trace, shade, composite
    o, d = camera_rays(eye, TARGET, size=(W, H))
    ext = pts.reshape(-1, 3).max(axis=0) - pts.reshape(-1, 3).min(axis=0)
    with SegmentCaster(pts, 0.01 * float(np.sqrt(np.sum(ext * ext)))) as sc:
        h = sc.trace(o, d, max_hits=2)
        lay = sc.shade(h, o, d, vals)
    assert np.array_equal(img, composite_layers(lay).reshape(H, W, 4)) and np.array_equal(depth, h.t[:, 0].reshape(H, W))
    bare, _ = render_lines(pts, eye, TARGET, **kw)           # without values: the table's first colour (black), opaque
    assert np.array_equal(bare[..., 3], img[..., 3]) and not bare[..., :3].any()
