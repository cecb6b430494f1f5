"""SegmentCaster / segments / curve_segments / merge_layers / render_lines / render_curve and the `lines` keywords of
render_figure on the CPU: every argument check raised before the library is touched, the empty soup without a device, and
the NumPy twin (tests/tubes_twin.py) the GPU tests compare against, itself pinned on closed forms.  The cases of
tests/test_gpu_tubes.py are defined here, so that the margin condition their comparisons rely on is checked without a
GPU, on the twin alone.
"""
import math

import numpy as np
import pytest

import mgb_amd as m
from mgb_amd.contour import Contour
from mgb_amd.raycast import camera_rays
from mgb_amd.streamlines import Streamlines
from mgb_amd.surface import render_figure
from mgb_amd.tubes import (SegmentCaster, TubeHits, curve_segments, default_radius, merge_layers, render_curve,
                           render_lines, segments)
from test_surface import MARGIN, rays65, UNIT
from tubes_twin import (CAP_A, CAP_B, EPS, NONE, SIDE, margin_twin, normalize_twin, pairs_twin, piece_of, s_bound,
                        shade_twin, t_bound, trace_twin)

# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_tubes.py
# ---------------------------------------------------------------------------------------------------------------------

SEG = np.array([[0.31, 0.36, 0.22], [0.68, 0.59, 0.79]])
NRAYS = (1, 64, 65)
HITS = (1, 4, 8)
FAR = np.array([1000.0, -1000.0, 1000.0])


def helix():
    """A 96-segment polyline winding three times through the unit box."""
    i = np.arange(97)
    th = 3.0 * 2.0 * math.pi * i / 96.0
    p = np.stack([0.5 + 0.35 * np.cos(th), 0.5 + 0.35 * np.sin(th), 0.1 + 0.8 * i / 96.0], axis=1)
    return np.stack([p[:-1], p[1:]], axis=1)


HELIX_R = 0.03
HELIX_WINDOW = (0.2, 3.3)


def helix_rays():
    """65 rays: five hand-placed ones, then the 60 rays of a 10 x 6 camera."""
    P = helix()
    a0, b0 = P[0]
    u0 = (b0 - a0) / np.linalg.norm(b0 - a0)
    mid20, mid36 = 0.5 * (P[20, 0] + P[20, 1]), 0.5 * (P[36, 0] + P[36, 1])       # half a turn apart
    radial = (mid20 - mid36) / np.linalg.norm(mid20 - mid36)
    mid50 = 0.5 * (P[50, 0] + P[50, 1])
    hand = [
        (a0 - 0.5 * u0, b0 - a0),                                  # parallel to segment 0's axis, into its free cap
        (mid50 + np.array([0.01, 0.0, 0.004]), (0.3, 0.5, -0.4)),  # origin inside capsule 50
        ((-1.0, -1.0, 2.0), (0.0, 0.0, 1.0)),                      # a complete miss
        (mid20 + 0.13 * radial, -radial),                          # its nearest hit lies before t_min; it goes on to 36
        ((0.5, 0.5, 0.92), (0.0, 0.0, 1.0)),                       # leaves the grid box at once
    ]
    o, d = camera_rays((2.2, -1.9, 1.55), (0.5, 0.5, 0.5), size=(10, 6), fov=17.0)
    o = np.concatenate([np.array([h[0] for h in hand], dtype=np.float64), o])
    d = np.concatenate([np.array([h[1] for h in hand], dtype=np.float64), d])
    assert o.shape == (65, 3)
    return o, d


def star():
    """40 segments through the point (0.5, 0.5, 0.5)."""
    rng = np.random.default_rng(11)
    u = rng.standard_normal((40, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    L = rng.uniform(0.25, 0.45, size=(40, 1))
    c = np.array([0.5, 0.5, 0.5])
    return np.stack([c - L * u, c + L * u], axis=1)


def random_segments(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.15, 0.85, size=(n, 1, 3))
    return np.clip(c + 0.1 * rng.standard_normal((n, 2, 3)), 0.0, 1.0)


def radii_spread(n):
    return 0.002 * 100.0 ** (np.arange(n) / (n - 1.0))


def dup_segments():
    """The same segment twice, and one behind it."""
    return np.stack([SEG, SEG, SEG + np.array([0.07, -0.05, -0.3])])


def _unit(points, radii, window=(0.02, 2.35)):
    o, d = rays65(*UNIT)
    return points, radii, o, d, window[0], window[1]


def _helix(shift=None):
    o, d = helix_rays()
    P = helix()
    if shift is not None:
        P, o = P + shift, o + shift
    return P, HELIX_R, o, d, HELIX_WINDOW[0], HELIX_WINDOW[1]


# name -> (points, radii, o, d, t_min, t_max); "dup" is excluded from the margin condition
GPU_CASES = {
    "one": lambda: _unit(SEG[None].copy(), 0.08),
    "one_sphere": lambda: _unit(np.stack([SEG[0], SEG[0]])[None].copy() + 0.2, 0.17),
    "helix": lambda: _helix(),
    "star": lambda: _unit(star(), 0.012),
    "radii": lambda: _unit(random_segments(48, 3), radii_spread(48)),
    "far": lambda: _helix(FAR),
    "dup": lambda: _unit(dup_segments(), 0.06),
}
TIES = ("dup",)


def case_tubes(name):
    return GPU_CASES[name]()


def end_values(points):
    """(S, 2): a smooth function of the end points."""
    P = points - np.floor(points.min())
    return np.sin(1.3 * P[..., 0] + 0.4) * np.cos(0.9 * P[..., 1] - 0.2) + 0.35 * np.sin(1.1 * P[..., 2] + 0.3)


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_gpu_cases_meet_the_margin_condition_on_the_twin(name):
    pts, rad, o, d, t_min, t_max = case_tubes(name)
    tw = trace_twin(pts, rad, o, d, t_min, t_max, 8)
    margin, gap = margin_twin(tw.pairs, t_min, t_max)
    nh = tw.pairs.hit.sum(axis=1)
    pieces = [int((tw.piece == p).sum()) for p in (SIDE, CAP_A, CAP_B)]
    print(f"{name}: S = {pts.shape[0]}, rays hit {int((nh > 0).sum())}/65, most hits {int(nh.max())}, side / cap a / cap b "
          f"{pieces}, margin {margin:.3e}, gap {gap:.3e}")
    assert np.isfinite(pts).all() and o.shape == (65, 3)
    assert nh[0] > 0, "the first ray (the 1-ray bundle) hits"
    assert (nh > 0).sum() >= 3 and (nh == 0).any(), "hits and misses"
    if name in TIES:
        assert gap == 0.0, "the duplicate case has ties in t"
        return
    assert margin > MARGIN and gap > MARGIN, (margin, gap)


def test_the_cases_hold_what_they_are_meant_to():
    # helix: the five hand-placed rays do what they are placed for
    pts, rad, o, d, t_min, t_max = case_tubes("helix")
    tw = trace_twin(pts, rad, o, d, t_min, t_max, 8)
    pr = tw.pairs
    assert tw.segment[0, 0] == 0 and tw.piece[0, 0] == CAP_A and pr.A[0, 0] <= 1e-12 * pr.baba[0, 0], "into the free cap"
    assert abs(tw.t[0, 0] - (0.5 - rad)) <= 1e-12
    assert pr.t[1, 50] < 0.0 and not pr.hit[1, 50], "the origin lies inside capsule 50, which is not hit"
    assert not pr.hit[2].any() and not pr.hit[4].any(), "a complete miss; a ray leaving the box at once"
    assert 0.0 < pr.t[3, 20] < t_min and not pr.hit[3, 20] and pr.hit[3, 36], "the window cuts the nearest hit away"
    assert (pr.hit & (pr.piece == SIDE)).any() and (pr.t[pr.piece != NONE] > t_max).any()
    far = trace_twin(*case_tubes("far")[:4], t_min, t_max, 8)
    assert np.array_equal(far.segment, tw.segment), "the translated case hits the same segments"
    # star: one ray meets more than eight capsules, so K = 8 truncates
    pts, rad, o, d, t_min, t_max = case_tubes("star")
    assert pairs_twin(pts, rad, o, normalize_twin(d), t_min, t_max).hit.sum(axis=1).max() > 8
    # radii: a factor of 100, and both the thinnest and the thickest tenth are hit
    pts, rad, o, d, t_min, t_max = case_tubes("radii")
    tw = trace_twin(pts, rad, o, d, t_min, t_max, 8)
    assert rad.max() / rad.min() == pytest.approx(100.0) and (tw.segment >= 43).any()
    assert (tw.piece == SIDE).any() and ((tw.piece == CAP_A) | (tw.piece == CAP_B)).any()
    # one_sphere: only cap a reports
    tw = trace_twin(*case_tubes("one_sphere"), 8)
    assert set(np.unique(tw.piece)) == {NONE, CAP_A}


# ---------------------------------------------------------------------------------------------------------------------
# the twin on closed forms
# ---------------------------------------------------------------------------------------------------------------------

ZCAP = np.array([[[0.0, 0.0, -1.0], [0.0, 0.0, 1.0]]])        # a capsule around the z axis


def test_twin_ray_along_x_hits_the_side_at_distance_minus_radius():
    for r, x0, z in ((0.25, 3.0, 0.5), (0.5, -7.0, -0.75), (0.125, 2.0, 0.0)):
        tw = trace_twin(ZCAP, r, [[x0, 0.0, z]], [[-x0, 0.0, 0.0]], 0.0, math.inf, 1)
        assert tw.segment[0, 0] == 0 and tw.piece[0, 0] == SIDE
        assert abs(tw.t[0, 0] - (abs(x0) - r)) <= 4 * EPS * abs(x0)
        assert abs(tw.s[0, 0] - (z + 1.0) / 2.0) <= 4 * EPS
    # beyond the end of the segment the cap is hit instead, later than the cylinder would be
    tw = trace_twin(ZCAP, 0.25, [[3.0, 0.0, 1.125]], [[-1.0, 0.0, 0.0]], 0.0, math.inf, 1)
    assert tw.piece[0, 0] == CAP_B and tw.s[0, 0] == 1.0
    assert abs(tw.t[0, 0] - (3.0 - math.sqrt(0.25 ** 2 - 0.125 ** 2))) <= 8 * EPS * 3.0
    assert trace_twin(ZCAP, 0.25, [[3.0, 0.0, 1.3]], [[-1.0, 0.0, 0.0]], 0.0, math.inf, 1).segment[0, 0] == -1


def test_twin_ray_down_the_axis_hits_the_cap():
    tw = trace_twin(ZCAP, 0.25, [[0.0, 0.0, 4.0]], [[0.0, 0.0, -2.0]], 0.0, math.inf, 1)
    assert tw.pairs.A[0, 0] == 0.0, "parallel to the axis: the side takes no part"
    assert tw.piece[0, 0] == CAP_B and tw.s[0, 0] == 1.0 and abs(tw.t[0, 0] - (3.0 - 0.25)) <= 4 * EPS * 3.0
    tw = trace_twin(ZCAP, 0.25, [[0.0, 0.0, -4.0]], [[0.0, 0.0, 1.0]], 0.0, math.inf, 1)
    assert tw.piece[0, 0] == CAP_A and tw.s[0, 0] == 0.0 and abs(tw.t[0, 0] - (3.0 - 0.25)) <= 4 * EPS * 3.0


def test_twin_equal_end_points_are_a_sphere():
    c = np.array([0.5, -0.25, 2.0])
    tw = trace_twin(np.stack([c, c])[None], 0.5, [c + [0.0, 5.0, 0.0], c + [3.0, 0.0, 0.3]], [[0.0, -1.0, 0.0], [-1.0, 0.0, 0.0]],
                    0.0, math.inf, 2)
    assert tw.pairs.A[0, 0] == 0.0 and tw.segment[:, 0].tolist() == [0, 0] and tw.segment[:, 1].tolist() == [-1, -1]
    assert (tw.piece[:, 0] == CAP_A).all() and (tw.s[:, 0] == 0.0).all(), "cap a wins the tie with cap b"
    assert abs(tw.t[0, 0] - 4.5) <= 8 * EPS * 5 and abs(tw.t[1, 0] - (3.0 - 0.4)) <= 8 * EPS * 3


def test_twin_origin_inside_gives_no_hit_and_the_window_is_inclusive():
    inside = trace_twin(ZCAP, 0.25, [[0.1, 0.0, 0.3], [0.0, 0.1, 1.1]], [[1.0, 0.0, 0.0], [0.0, 0.3, 1.0]], 0.0, math.inf, 1)
    assert (inside.segment == -1).all() and np.isinf(inside.t).all() and np.isnan(inside.s).all()
    assert (inside.pairs.t < 0.0).all(), "the entry lies behind the origin"
    o, d = [[3.0, 0.0, 0.5]], [[-1.0, 0.0, 0.0]]                     # enters at t = 2.75 exactly
    assert trace_twin(ZCAP, 0.25, o, d, 2.75, 9.0, 1).segment[0, 0] == 0
    assert trace_twin(ZCAP, 0.25, o, d, 0.0, 2.75, 1).segment[0, 0] == 0
    assert trace_twin(ZCAP, 0.25, o, d, 2.75 + 1e-9, 9.0, 1).segment[0, 0] == -1, "the exit point is never reported"
    assert trace_twin(ZCAP, 0.25, o, d, 0.0, 2.75 - 1e-9, 1).segment[0, 0] == -1


def test_twin_keeps_the_nearest_in_order_and_ties_go_to_the_lower_index():
    x = np.array([0.7, 0.1, 0.9, 0.3, 1.0, 0.2, 0.8, 0.4, 0.6, 0.5])
    pts = np.stack([ZCAP[0] + np.array([xx, 0.0, 0.0]) for xx in x])
    tw = trace_twin(pts, 0.01, [[2.0, 0.0, 0.25]], [[-3.0, 0.0, 0.0]], 0.0, math.inf, 4)
    assert tw.segment.tolist() == [[4, 2, 6, 0]]
    # h is a difference of terms of size dist^2 that leaves r^2: t carries about eps dist^2 / r
    assert np.abs(tw.t[0] - (2.0 - x[[4, 2, 6, 0]] - 0.01)).max() <= 8 * EPS * 2.0 ** 2 / 0.01
    tw = trace_twin(np.concatenate([ZCAP, ZCAP, ZCAP]), 0.25, [[3.0, 0.0, 0.5]], [[-1.0, 0.0, 0.0]], 0.0, math.inf, 2)
    assert tw.segment.tolist() == [[0, 1]] and tw.t[0, 0] == tw.t[0, 1] == 2.75


def test_twin_bounds_and_piece_of():
    tw = trace_twin(*case_tubes("radii"), 4)
    bt, bs = t_bound(tw), s_bound(tw)
    hit = tw.segment >= 0
    assert (bt[hit] > 0).all() and (bt[hit] < 1e-12).all() and (bt[~hit] == 0).all()
    assert (bs[tw.piece == SIDE] > 0).all() and (bs[tw.piece != SIDE] == 0).all() and bs.max() < 1e-11
    assert np.array_equal(piece_of(tw.s, tw.segment), tw.piece)


def test_twin_shade_formula():
    o = np.array([[3.0, 0.0, 0.5], [0.0, 0.0, 4.0]])
    d = np.array([[-1.0, 0.0, 0.0], [0.0, 0.0, -2.0]])
    tw = trace_twin(ZCAP, 0.25, o, d, 0.0, math.inf, 1)
    table = np.array([[0.0, 0.0, 1.0, 0.5], [1.0, 0.5, 0.0, 1.5]])
    L = shade_twin(ZCAP, o, normalize_twin(d), tw.t, tw.segment, tw.s, np.array([[0.0, 2.0]]), table, 0.0, 2.0, 0.3)
    for r, c in enumerate((1.5, 2.0)):                        # s = 0.75 on the side, 1 on cap b; head-on: |nn . dn| = 1
        w = c / 2.0
        alpha = min(1.0, 0.5 + w)
        assert np.abs(L[r, 0] - [alpha * w, alpha * 0.5 * w, alpha * (1.0 - w), alpha]).max() <= 8 * EPS
    o2 = np.array([[3.0, 0.125, 0.5]])                         # off centre: nn . dn = -cos(asin(0.5))
    tw2 = trace_twin(ZCAP, 0.25, o2, d[:1], 0.0, math.inf, 1)
    L2 = shade_twin(ZCAP, o2, normalize_twin(d[:1]), tw2.t, tw2.segment, tw2.s, np.array([[1.0, 1.0]]),
                    np.array([[1.0, 1.0, 1.0, 1.0]] * 2), 0.0, 2.0, 0.3)
    assert abs(L2[0, 0, 0] - (0.3 + 0.7 * math.sqrt(0.75))) <= 8 * EPS and L2[0, 0, 3] == 1.0
    missing = shade_twin(ZCAP, o, normalize_twin(d), tw.t, np.array([[-1], [0]], dtype=np.int32), tw.s,
                         np.array([[0.0, np.nan]]), table, 0.0, 2.0, 0.3)
    assert np.array_equal(missing, np.zeros((2, 1, 4)))       # a missing hit, a non-finite value


# ---------------------------------------------------------------------------------------------------------------------
# segments, curve_segments, merge_layers
# ---------------------------------------------------------------------------------------------------------------------

def test_names_are_exported():
    for name in ("SegmentCaster", "TubeHits", "segments", "curve_segments", "merge_layers", "render_lines", "render_curve"):
        assert getattr(m, name) is getattr(m.tubes, name), name


def _lines3():
    pts = np.full((3, 5, 3), np.nan)
    pts[0, :4] = np.arange(12.0).reshape(4, 3)
    pts[1, :1] = [9.0, 9.0, 9.0]                               # a single point: no segment
    pts[2, :5] = 100.0 + np.arange(15.0).reshape(5, 3)
    return Streamlines(pts, np.array([4, 1, 5], dtype=np.int32), np.zeros(3, dtype=np.int32))


def test_segments_of_streamlines_contours_arrays_and_lists():
    st = _lines3()
    P, V = segments(st)
    assert V is None and P.shape == (7, 2, 3)
    assert np.array_equal(P[:3, 0], st.points[0, :3]) and np.array_equal(P[:3, 1], st.points[0, 1:4])
    assert np.array_equal(P[3:, 0], st.points[2, :4]) and np.array_equal(P[3:, 1], st.points[2, 1:5])
    vals = np.arange(15.0).reshape(3, 5)
    P, V = segments(st, vals)
    assert np.array_equal(V, [[0, 1], [1, 2], [2, 3], [10, 11], [11, 12], [12, 13], [13, 14]])
    empty = Streamlines(np.full((2, 3, 3), np.nan), np.zeros(2, np.int32), np.zeros(2, np.int32))
    assert segments(empty)[0].shape == (0, 2, 3)
    cp = np.arange(12.0).reshape(2, 2, 3)
    carried = np.arange(8.0).reshape(2, 2, 2)
    con = Contour(cp, np.zeros(2, np.int32), np.zeros(2, np.int32), carried, 1)
    P, V = segments(con)
    assert np.array_equal(P, cp) and np.array_equal(V, carried[..., 0])
    bare = Contour(cp, np.zeros(2, np.int32), np.zeros(2, np.int32), None, 1)
    assert segments(bare)[1] is None and np.array_equal(segments(bare, [5.0, 6.0])[1], [[5, 5], [6, 6]])
    P, V = segments(cp, np.ones((2, 2)))
    assert np.array_equal(P, cp) and np.array_equal(V, np.ones((2, 2)))
    P, V = segments([st, bare, cp])
    assert P.shape == (11, 2, 3) and V is None and np.array_equal(P[7:9], cp) and np.array_equal(P[9:], cp)
    P, V = segments([st, con], [vals, None])
    assert P.shape == (9, 2, 3) and V.shape == (9, 2) and np.array_equal(V[7:], carried[..., 0])
    assert segments([])[0].shape == (0, 2, 3) and segments([])[1] is None


def test_segments_refusals():
    flat = Contour(np.zeros((1, 2, 2)), np.zeros(1, np.int32), np.zeros(1, np.int32), None, 1)
    st2 = Streamlines(np.zeros((1, 3, 2)), np.array([3], np.int32), np.zeros(1, np.int32))
    tri = Contour(np.zeros((1, 3, 3)), np.zeros(1, np.int32), np.zeros(1, np.int32), None, 1)
    cp = np.zeros((2, 2, 3))
    for lines, values, match in [
        (flat, None, "the lines of a flat 2-D mesh are not in R\\^3"),
        (st2, None, "the lines of a flat 2-D mesh are not in R\\^3"),
        (np.zeros((4, 2, 2)), None, "the lines of a flat 2-D mesh are not in R\\^3"),
        ([cp, flat], None, "the lines of a flat 2-D mesh are not in R\\^3"),
        (tri, None, r"a Contour must hold level curves in R\^3, \(S, 2, 3\)"),
        (np.zeros((4, 3)), None, r"lines must be a Streamlines, a Contour, an \(S, 2, 3\) array or a list"),
        ("abc", None, r"lines must be a Streamlines, a Contour, an \(S, 2, 3\) array or a list"),
        (cp, np.zeros(3), r"values must be \(2,\) or \(2, 2\)"),
        (_lines3(), np.zeros((3, 4)), r"values of a Streamlines must be \(3, 5\)"),
        ([cp, cp], np.zeros((4, 2)), "values for a list of lines must be a list with one entry per item"),
        ([cp, cp], [np.zeros(2), None], "some items of lines have values and some have none"),
    ]:
        with pytest.raises(ValueError, match="segments: .*" + match):
            segments(lines, values)


def circle3(n=8, k=2):
    """An n-element Q_k circle in R^3 (tilted), nodes equally spaced in angle."""
    th = 2.0 * math.pi * (np.arange(n)[None, :] + np.linspace(0.0, 1.0, k + 1)[:, None]) / n      # (k + 1, n)
    return np.stack([np.cos(th), np.sin(th), 0.3 * np.cos(th)], axis=2)


def test_curve_segments_join_the_nodes_of_every_element():
    g3 = m.fem1d(k=2, K=circle3(), ambient=3)
    z = np.arange(24.0)
    P, V = curve_segments(g3, z)
    assert P.shape == (16, 2, 3) and V.shape == (16, 2)
    X = g3.xflat
    for el in range(8):
        for j in range(2):                                   # create_vtk_line_connectivity: base + j, base + j + 1
            i = el * 2 + j
            assert np.array_equal(P[i, 0], X[el * 3 + j]) and np.array_equal(P[i, 1], X[el * 3 + j + 1])
            assert V[i].tolist() == [el * 3 + j, el * 3 + j + 1]
    g2 = m.fem1d(k=2, K=circle3()[..., :2], ambient=2)
    P2, V2 = curve_segments(g2, z, height_scale=0.5)
    assert np.array_equal(P2[..., :2], P[..., :2]) and np.array_equal(P2[..., 2], 0.5 * V2) and np.array_equal(V2, V)


def test_curve_segments_refusals():
    with pytest.raises(ValueError, match=r"curve_segments: a flat fem1d geometry \(e = 1\)"):
        curve_segments(m.fem1d(nodes=np.linspace(-1, 1, 4)), np.zeros(6))
    for geom, name in [(m.fem2d(k=1), "fem2d"), (m.fem3d(k=1), "fem3d"), (m.fem2d_P1(), "fem2d_P1"), (m.fem2d_P2(), "fem2d_P2"),
                       (m.spectral1d(n=4), "spectral1d"), (m.spectral2d(n=4), "spectral2d")]:
        with pytest.raises(ValueError, match=rf"curve_segments: {name} geometries are not supported"):
            curve_segments(geom, np.zeros(4))
    g3 = m.fem1d(k=2, K=circle3(), ambient=3)
    with pytest.raises(ValueError, match="curve_segments: z must be a vector of 24 values"):
        curve_segments(g3, np.zeros(23))
    with pytest.raises(ValueError, match="curve_segments: height_scale must be a finite number"):
        curve_segments(g3, np.zeros(24), height_scale=np.inf)


def test_merge_layers_sorts_stably_and_cuts():
    inf = np.inf
    t1 = np.array([[1.0, 3.0, inf], [2.0, inf, inf]])
    t2 = np.array([[3.0, 4.0], [inf, inf]])
    l1 = np.arange(24.0).reshape(2, 3, 4)
    l2 = 100.0 + np.arange(16.0).reshape(2, 2, 4)
    t, layer = merge_layers((t1, l1), (t2, l2))
    assert t.shape == (2, 5) and layer.shape == (2, 5, 4)
    assert np.array_equal(t, [[1.0, 3.0, 3.0, 4.0, inf], [2.0, inf, inf, inf, inf]])
    assert np.array_equal(layer[0], [l1[0, 0], l1[0, 1], l2[0, 0], l2[0, 1], l1[0, 2]]), "the tie at 3 keeps argument order"
    assert np.array_equal(layer[1], [l1[1, 0], l1[1, 1], l1[1, 2], l2[1, 0], l2[1, 1]])
    t, layer = merge_layers((t2, l2), (t1, l1), max_hits=3)
    assert np.array_equal(t, [[1.0, 3.0, 3.0], [2.0, inf, inf]])
    assert np.array_equal(layer[0], [l1[0, 0], l2[0, 0], l1[0, 1]]), "the other order of the tie"
    big = merge_layers((np.zeros((1, 8)), np.zeros((1, 8, 4))), (np.ones((1, 8)), np.ones((1, 8, 4))))
    assert big[0].shape == (1, 8) and not big[0].any(), "the default cut is min(8, sum K_i)"
    for args, kw, match in [
        ((), {}, "at least one"),
        ((3.0,), {}, r"argument 0 must be a \(t, layer\) pair"),
        (((t1, l2),), {}, r"argument 0 must be t \(R, K\) and layer \(R, K, 4\)"),
        (((t1, l1), (t2[:1], l2[:1])), {}, "argument 1 holds 1 rays, argument 0 holds 2"),
        (((np.full((2, 3), np.nan), l1),), {}, "has a NaN"),
        (((t1, l1),), dict(max_hits=9), r"max_hits must be an integer in 1\.\.8"),
        (((np.zeros((1, 8)), np.zeros((1, 8, 4))),) * 3, {}, "at most 16 can be merged"),
    ]:
        with pytest.raises(ValueError, match="merge_layers: .*" + match):
            merge_layers(*args, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the empty soup and every refusal, without a device
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library or open a device context fails the test."""
    from mgb_amd import device

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(device, "load_library", boom)
    monkeypatch.setattr(device, "HipContext", boom)


O2, D2 = np.zeros((2, 3)), np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 1.0]])
NOSEG = np.zeros((0, 2, 3))


def test_empty_soup_misses_without_a_device(no_library):
    with SegmentCaster(NOSEG, 0.1) as sc:
        h = sc.trace(O2, D2, max_hits=3)
        assert isinstance(h, TubeHits) and h.t.shape == (2, 3) and np.isinf(h.t).all()
        assert (h.segment == -1).all() and h.segment.dtype == np.int32 and np.isnan(h.s).all()
        assert np.array_equal(sc.shade(h, O2, D2, np.zeros((0, 2))), np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="SegmentCaster: the caster is closed"):
        sc.trace(O2, D2)
    img, depth = render_lines(NOSEG, (3, 2, 1), (0, 0, 0), size=(4, 3))
    assert img.shape == (3, 4, 4) and not img.any() and depth.shape == (3, 4) and np.isinf(depth).all()
    img, depth = render_lines([], (3, 2, 1), (0, 0, 0), size=(4, 3))
    assert img.shape == (3, 4, 4) and not img.any()


@pytest.mark.parametrize("points, radius, match", [
    (np.zeros((2, 3)), 0.1, r"points must be \(S, 2, 3\)"),
    (np.zeros((2, 3, 3)), 0.1, r"points must be \(S, 2, 3\)"),
    (np.full((1, 2, 3), np.nan), 0.1, "every entry of points must be finite"),
    (np.zeros((2, 2, 3)), 0.0, "every radius must be finite and positive"),
    (np.zeros((2, 2, 3)), -1.0, "every radius must be finite and positive"),
    (np.zeros((2, 2, 3)), np.inf, "every radius must be finite and positive"),
    (np.zeros((2, 2, 3)), [0.1, np.nan], "every radius must be finite and positive"),
    (np.zeros((2, 2, 3)), [0.1, 0.2, 0.3], r"radius must be a positive finite number or \(2,\) of them"),
    (np.zeros((2, 2, 3)), "thick", r"radius must be a positive finite number or \(2,\) of them"),
])
def test_points_and_radius_refusals(no_library, points, radius, match):
    with pytest.raises(ValueError, match="SegmentCaster: .*" + match):
        SegmentCaster(points, radius)


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
    (dict(t_min=1.0, t_max=1.0), "t_max must be greater than t_min"),
    (dict(t_min=-np.inf), "t_min must be finite"),
    (dict(t_max=np.nan), "t_max must be greater than t_min"),
    (dict(t_min="a"), "t_min and t_max must be numbers"),
])
def test_trace_refusals(no_library, kw, match):
    args = dict(o=O2, d=D2)
    args.update(kw)
    with SegmentCaster(NOSEG, 0.1) as sc:
        with pytest.raises(ValueError, match="SegmentCaster.trace: .*" + match):
            sc.trace(**args)


def test_shade_refusals(no_library):
    with SegmentCaster(NOSEG, 0.1) as sc:
        h = sc.trace(O2, D2, max_hits=2)
        V = np.zeros((0, 2))
        zero = np.zeros((2, 2), np.int32)
        for args, kw, match in [
            (((h.t, h.segment), O2, D2, V), {}, "hits must be what trace"),
            ((h, O2[:1], D2[:1], V), {}, "hits hold"),
            ((h, O2, np.zeros((2, 3)), V), {}, "a ray direction d is zero"),
            ((h, np.full((2, 3), np.nan), D2, V), {}, "every ray origin o must be finite"),
            ((h, O2, D2, np.zeros((1, 2))), {}, r"values must be \(0, 2\)"),
            ((TubeHits(h.t, zero, h.s), O2, D2, V), {}, r"an index outside -1\.\.-1"),
            ((TubeHits(h.t, h.segment, h.s[:, :1]), O2, D2, V), {}, "hits.t and hits.s must have the shape"),
            ((h, O2, D2, V), dict(transfer=np.zeros((1, 4))), r"transfer must be \(K, 4\) with K >= 2"),
            ((h, O2, D2, V), dict(transfer=np.full((3, 4), np.nan)), "every transfer entry must be finite"),
            ((h, O2, D2, V), dict(clim=(1.0, 1.0)), "clim must be finite with lo < hi"),
            ((h, O2, D2, V), dict(ambient=1.5), r"ambient must be a number in \[0, 1\]"),
        ]:
            with pytest.raises(ValueError, match="SegmentCaster.shade: .*" + match):
                sc.shade(*args, **kw)


def test_shade_refuses_unusable_hits_before_the_device(monkeypatch):
    """A caster with segments, its device handle faked: the checks of hits run before the library is called."""
    sc = SegmentCaster(NOSEG, 0.1)
    sc.nsegments = 2
    seg = np.array([[0, -1], [1, -1]], np.int32)
    t = np.array([[1.0, np.inf], [2.0, np.inf]])
    for hits, match in [
        (TubeHits(np.array([[np.inf, np.inf], [2.0, np.inf]]), seg, np.array([[0.5, np.nan], [0.0, np.nan]])), "finite hits.t"),
        (TubeHits(t, seg, np.array([[1.5, np.nan], [0.0, np.nan]])), r"hits.s in \[0, 1\]"),
        (TubeHits(t, seg, np.array([[np.nan, np.nan], [0.0, np.nan]])), r"hits.s in \[0, 1\]"),
    ]:
        with pytest.raises(ValueError, match="SegmentCaster.shade: .*" + match):
            sc.shade(hits, O2, D2, np.zeros((2, 2)))


def test_render_lines_and_render_curve_refusals(no_library):
    cam = dict(eye=(3, 2, 1), target=(0, 0, 0), size=(4, 3))
    seg = SEG[None]
    for lines, kw, match in [
        (np.zeros((1, 2, 2)), {}, "the lines of a flat 2-D mesh are not in R\\^3"),
        (seg, dict(values=np.zeros(2)), r"values must be \(1,\) or \(1, 2\)"),
        (seg, dict(max_hits=0), r"max_hits must be an integer in 1\.\.8"),
        (seg, dict(ambient=-0.1), "ambient must be a number"),
        (seg, dict(transfer=np.zeros((2, 3))), r"transfer must be \(K, 4\)"),
        (seg, dict(radius=0.0), "every radius must be finite and positive"),
        (seg, dict(radius=[0.1, 0.2]), r"radius must be a positive finite number or \(1,\) of them"),
        (np.stack([SEG[0], SEG[0]])[None], {}, "span no extent to take the default radius from"),
        (np.full((1, 2, 3), np.inf), {}, "non-finite points"),
        (seg, dict(values=np.ones(1)), "values is constant"),
        (seg, dict(values=np.full(1, np.nan)), "values has no finite entry"),
    ]:
        with pytest.raises(ValueError, match="render_lines: .*" + match):
            render_lines(lines, **cam, **kw)
    with pytest.raises(ValueError, match="camera_rays: size"):
        render_lines(seg, (3, 2, 1), (0, 0, 0), size=(0, 3))
    g3 = m.fem1d(k=2, K=circle3(), ambient=3)
    with pytest.raises(ValueError, match="render_curve: z must be a vector of 24 values"):
        render_curve(g3, np.zeros(3), **cam)
    with pytest.raises(ValueError, match="render_curve: fem3d geometries are not supported"):
        render_curve(m.fem3d(k=1), np.zeros(8), **cam)
    with pytest.raises(ValueError, match=r"render_curve: a flat fem1d geometry \(e = 1\)"):
        render_curve(m.fem1d(), np.zeros(2), **cam)
    with pytest.raises(ValueError, match="render_curve: z is constant|render_curve: values is constant"):
        render_curve(g3, np.ones(24), **cam)
    assert default_radius(seg) == pytest.approx(0.01 * np.linalg.norm(SEG[1] - SEG[0]))


def test_render_figure_line_refusals(no_library):
    g3 = m.fem3d(k=1)
    u = g3.xflat @ np.array([1.0, 2.0, 4.0])
    cam = dict(eye=(3, 2, 1), target=(0, 0, 0), size=(4, 3))
    seg = SEG[None]
    for kw, match in [
        (dict(lines=np.zeros((1, 2, 2))), "render_figure: the lines of a flat 2-D mesh are not in R\\^3"),
        (dict(lines=[0.1, 0.2]), r"render_figure: lines must be a Streamlines, a Contour, an \(S, 2, 3\) array or a list"),
        (dict(lines=seg, line_radius=-1.0), "render_figure: every line_radius must be finite and positive"),
        (dict(lines=seg, line_radius=[1.0, 2.0]), r"render_figure: line_radius must be a positive finite number or \(1,\)"),
        (dict(lines=seg, line_color=(0.0, 1.0)), "render_figure: line_color must be three finite numbers"),
        (dict(lines=seg, line_color=(0.0, np.nan, 1.0)), "render_figure: line_color must be three finite numbers"),
        (dict(lines=np.full((1, 2, 3), np.nan)), "render_figure: lines have non-finite points"),
    ]:
        with pytest.raises(ValueError, match=match):
            render_figure(g3, u, **cam, **kw)
    from test_manifold_post import sphere
    gs = sphere(1, 1)
    us = gs.xflat @ np.array([1.0, 2.0, 4.0])
    for kw, match in [
        (dict(lines=[0.1, np.nan]), "render_figure: every level value of lines must be finite"),
        (dict(lines=[0.1], line_radius=[0.1, 0.2]), "render_figure: line_radius must be a positive finite number when lines"),
        (dict(lines=[0.1], line_color="red"), "render_figure: line_color must be three finite numbers"),
        (dict(lines=np.zeros((1, 2, 2))), "render_figure: the lines of a flat 2-D mesh are not in R\\^3"),
    ]:
        with pytest.raises(ValueError, match=match):
            render_figure(gs, us, **cam, **kw)
